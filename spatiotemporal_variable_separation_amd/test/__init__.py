"""Evaluation entry points (reference: var_sep/test/*): `python -m spatiotemporal_variable_separation_amd.test.<dataset>.<script>`."""
