"""polus_amd.ir: retrieval models, trainers, indexes and searches.  `HybridSearch` and `fuse` (polus_amd/ir/fusion.py) are
exported here; they are resolved on first use, so importing one submodule does not import the others."""
__all__ = ["HybridSearch", "fuse"]


def __getattr__(name):
    if name in __all__:
        from . import fusion
        return getattr(fusion, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
