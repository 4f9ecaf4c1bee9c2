"""polus.ir.cross -> polus_amd.ir.cross (re-export; no counterpart module in the reference, which has no cross-encoder)."""
from polus_amd.ir import cross as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
