"""`sc.experimental`: the reference's experimental namespace (src/scanpy/experimental/__init__.py); here the analytic Pearson
residuals of `experimental.pp`."""
from __future__ import annotations

from . import pp

__all__ = ["pp"]
