"""WaveEq preparation: the simulations (gen_wave, on the device) and the WaveEq-100 pixel choice (gen_pixels, on the host)."""
