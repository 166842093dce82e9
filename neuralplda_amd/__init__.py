"""neuralplda_amd — MI355X-native (gfx950) Neural-PLDA scoring/training hot path.

The arithmetic lives in libnplda_hip.so (C ABI: include/nplda_hip.h; sources: csrc/*.hip);
this package is the host-side mirror of the reference's Python interface for that path.
"""
__version__ = "0.1.0"

_FEATURES = ("VadOptions", "PreparedFeatures", "prepare_features")


def __getattr__(name):
    """The feature front end (neuralplda_amd/features.py), resolved on first use: importing the package stays free of torch."""
    if name in _FEATURES:
        from . import features
        return getattr(features, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
