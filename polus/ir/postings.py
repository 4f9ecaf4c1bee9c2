"""polus.ir.postings -> polus_amd.ir.postings (re-export; no counterpart module in the reference, which has no lexical stage)."""
from polus_amd.ir import postings as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
