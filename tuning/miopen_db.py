"""Working copy of the committed MIOpen user database.

``tuning/miopen/`` holds the convolution solutions found once by
``bench.py --cudnn-benchmark`` so a fresh box reuses them.  MIOpen rewrites its
user database whenever it runs (new find results, the ``.time`` stamps), so
the benchmarks do not point ``MIOPEN_USER_DB_PATH`` at the committed files:
``user_db_path()`` copies them once into ``build/miopen_user_db/`` (untracked)
and returns that directory.  To commit new tuning results, copy the files back
from there.  No torch import here: the path must be set before MIOpen starts.

A checkout this user may not write to (built by someone else, read-only
mount) gets its working copy in the temporary directory instead, one per user
and checkout; if that cannot be written either, the committed directory is
used as it is, which MIOpen then only reads.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import tempfile

_HERE = os.path.dirname(os.path.abspath(__file__))
COMMITTED = os.path.join(_HERE, "miopen")
WORKING = os.path.join(os.path.dirname(_HERE), "build", "miopen_user_db")


def _fallback() -> str:
    uid = os.getuid() if hasattr(os, "getuid") else 0
    tag = hashlib.sha256(_HERE.encode()).hexdigest()[:12]
    return os.path.join(tempfile.gettempdir(), "gksgd_miopen_user_db_%d_%s" % (uid, tag))


def _prepare(working: str) -> str:
    """Create / complete one working copy (files already there are kept: they
    hold what MIOpen learnt since); OSError if it cannot be written."""
    os.makedirs(working, exist_ok=True)
    if not os.access(working, os.W_OK | os.X_OK):
        raise PermissionError("not writable: %s" % working)
    for name in sorted(os.listdir(COMMITTED)) if os.path.isdir(COMMITTED) else []:
        dst = os.path.join(working, name)
        if not os.path.exists(dst):
            # several ranks may start at once: copy aside, then rename into place
            tmp = "%s.%d.tmp" % (dst, os.getpid())
            shutil.copy2(os.path.join(COMMITTED, name), tmp)
            os.replace(tmp, dst)
    return working


def user_db_path(working: str = WORKING) -> str:
    """The directory for ``MIOPEN_USER_DB_PATH``: the first of ``working``
    and the per-user temporary copy that can be written, else the committed
    directory itself."""
    for cand in (working, _fallback()):
        try:
            return _prepare(cand)
        except OSError:
            continue
    return COMMITTED
