"""Training losses the controller resolves by name (``getattr(phyloss, config.loss)``; reference: pdecontrol/mbrl/mbrl.py:213-216)."""
