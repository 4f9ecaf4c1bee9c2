"""polus.ner.metrics -> polus_amd.ner.metrics (re-export)."""
from polus_amd.ner import metrics as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
