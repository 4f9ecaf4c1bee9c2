"""polus.ner.bio -> polus_amd.ner.bio (re-export)."""
from polus_amd.ner import bio as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
