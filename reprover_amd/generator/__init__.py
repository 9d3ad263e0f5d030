"""The reference's generator data and validation layers (generation/datamodule.py, generation/model.py,
generation/main.py) on the HIP engine.  Named ``generator`` so that it does not shadow ``reprover_amd.generation``."""
