"""Dataset preparation (reference: var_sep/preprocessing/*): `python -m spatiotemporal_variable_separation_amd.preprocessing.<dataset>.<script>`."""
