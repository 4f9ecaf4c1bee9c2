"""polus.ir.search -> polus_amd.ir.search (re-export)."""
from polus_amd.ir import search as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
