"""polus.ir.mining -> polus_amd.ir.mining (re-export; no counterpart module in the reference, which has no mining code)."""
from polus_amd.ir import mining as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
