"""polus.ir.fusion -> polus_amd.ir.fusion (re-export; no counterpart module in the reference, which has a single first stage)."""
from polus_amd.ir import fusion as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
