"""Module name `optim` -> sgc_amd.optim (drop-in shim).

Put dropin/ first on sys.path (or PYTHONPATH) and `from optim import LBFGS`
gives the device-resident L-BFGS with torch.optim.LBFGS's constructor, for the
reference's reddit.py:52 (`optim.LBFGS(model.parameters(), lr=1)`), and
`from optim import Adam` the device-resident Adam with torch.optim.Adam's
constructor and a run_epochs() for the loop of citation.py:41-50.  See
INTEGRATION.md.
"""
import os as _os
import sys as _sys

_ROOT = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
if _ROOT not in _sys.path:
    _sys.path.insert(0, _ROOT)

from sgc_amd.optim import *  # noqa: E402,F401,F403
from sgc_amd import optim as _impl  # noqa: E402

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
globals().update({n: getattr(_impl, n) for n in __all__})
