"""3D Chairs preparation: crop and Lanczos resize of the original renders (gen_chairs, on the device)."""
