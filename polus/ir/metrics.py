"""polus.ir.metrics -> polus_amd.ir.metrics (re-export)."""
from polus_amd.ir import metrics as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
