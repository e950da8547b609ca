"""The harness of the GPSGS_ACCELERATE hook tests (test_*_hook.py): each case runs in a fresh interpreter with the integration path -- the drop-in
directory ahead of the reference, the working directory a scratch copy of the reference's layout -- so that the import ORDER of the reference's
own files is what the hook has to cope with.  The reference is the checkout in the build container; `needs_ref` skips where there is none.
And the one pinned copy of the hook's table of names (NAMES, assert_the_names), which the module tests (test_*_module.py) share."""
import os
import subprocess
import sys
import textwrap

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refenv  # noqa: E402

REF = refenv.reference_dir()
needs_ref = pytest.mark.skipif(REF is None, reason="no reference checkout here")

# every name GPSGS_ACCELERATE accepts, in the order requested() answers in: (implied by "all", has a <name>_passthrough counter, counters from import)
NAMES = (("pack", (True, False, True)), ("loss", (True, True, True)), ("corr", (True, False, True)), ("upsample", (True, False, True)),
         ("unproject", (True, True, True)), ("splat", (False, False, True)), ("groupnorm", (False, True, True)), ("resblock", (False, True, True)),
         ("stemconv", (False, True, True)), ("gshead", (False, True, True)), ("conv3x3", (False, True, False)), ("conv1x1", (False, True, False)))


def assert_the_names(A):
    """Every name's place and kind, once for all the module tests: the whole known order, each name's three properties, and the three public tuples
    as what those properties make them (`calls` is left as it was found)."""
    known = tuple(n for n, _ in NAMES)
    keys = list(A.calls)
    try:
        assert A.requested(",".join(reversed(known))) == known
    finally:
        for k in [k for k in A.calls if k not in keys]:
            del A.calls[k]
    assert tuple(A.NAMES.items()) == NAMES
    assert A.FEATURES == tuple(n for n, (in_all, _, early) in NAMES if in_all) == A.requested("all")
    assert A.OPT_IN == tuple(n for n, (in_all, _, early) in NAMES if not in_all and early)
    assert A.BY_NAME == tuple(n for n, (in_all, _, early) in NAMES if not early) == ("conv3x3", "conv1x1")
    assert A.FEATURES + A.OPT_IN + A.BY_NAME == known


_PRELUDE = """
import os, sys
ROOT, REF = %r, %r
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refenv
refenv.activate(REF)
os.chdir(refenv.make_workdir(REF, %r))
"""
_built = False


def run(body, env_value, tmp_path):
    """The stdout of a child interpreter that ran `body` with GPSGS_ACCELERATE=env_value (None: unset); a non-zero exit status fails the test."""
    global _built
    if not _built:          # the conversions ask the library what it implements: every hook test file passes alone on a clean checkout
        import gps_gaussian_amd
        gps_gaussian_amd.build()
        _built = True
    code = (_PRELUDE % (ROOT, REF, str(tmp_path / "work"))) + textwrap.dedent(body)
    env = dict(os.environ)
    env.pop("GPSGS_ACCELERATE", None)
    if env_value is not None:
        env["GPSGS_ACCELERATE"] = env_value
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def lines(out, tag):
    return [l for l in out.splitlines() if tag in l.split(" ")[:2]]
