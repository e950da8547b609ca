"""CPU, no reference checkout needed: what the GPSGS_ACCELERATE hook (gps-gaussian_amd/accelerate.py) rebinds, wraps and counts for every
combination of the constructor-wrapping names -- `groupnorm`, `resblock`, `stemconv`, `gshead`, each with and without `all` -- on a stand-in
package this file writes itself: `core/extractor.py` (ResidualBlock, UnetExtractor) and `lib/gs_parm_network.py` (GSRegresser), with just the
members the hook looks at.  The expectations are spelled out from the rules of the hook's documentation, not recorded from a run.

The matrix runs in ONE child interpreter (fresh: the first case checks that nothing of the hook is imported while the variable is unset); every
case goes through the drop-in's `_bootstrap.submodule`, imports the stand-in anew and ends with `accelerate.uninstall()`.  A second child runs
restore() / uninstall(), two apply() calls in a row and the 16-try limit of late_apply()."""
import itertools
import json
import os
import subprocess
import sys
import textwrap

import pytest

import gps_gaussian_amd
from gps_gaussian_amd import accelerate as A

NAMES = ("groupnorm", "resblock", "stemconv", "gshead")
SUBSETS = [s for n in range(len(NAMES) + 1) for s in itertools.combinations(NAMES, n)]
# the variable's value per case; the unset case first, "all" second, "groupnorm" third (the child checks what is NOT imported by then)
CASES = [(s, with_all) for with_all in (False, True) for s in SUBSETS]
CASES.sort(key=lambda c: (c != ((), False), c != ((), True), c != (("groupnorm",), False)))


def _value(case):
    names = (("all",) if case[1] else ()) + case[0]
    return ",".join(names) if names else None


_EXTRACTOR = '''
import torch
from torch import nn


def _norm(kind, channels):
    return nn.GroupNorm(channels // 8, channels) if kind == "group" else nn.BatchNorm2d(channels)


class ResidualBlock(nn.Module):
    def __init__(self, c_in, c_out, norm="group", stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(c_in, c_out, 3, stride, 1)
        self.norm1 = _norm(norm, c_out)
        self.conv2 = nn.Conv2d(c_out, c_out, 3, 1, 1)
        self.norm2 = _norm(norm, c_out)
        self.downsample = None
        if stride != 1 or c_in != c_out:
            self.downsample = nn.Sequential(nn.Conv2d(c_in, c_out, 1, stride), _norm(norm, c_out))

    def forward(self, x):
        y = torch.relu(self.norm1(self.conv1(x)))
        y = torch.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return torch.relu(x + y)


class UnetExtractor(nn.Module):
    def __init__(self, in_channel=3):
        super().__init__()
        self.in_ds = nn.Sequential(nn.Conv2d(in_channel, 32, 5, 2, 2), nn.GroupNorm(4, 32), nn.ReLU())
        self.res1 = ResidualBlock(32, 32)
        self.res2 = ResidualBlock(32, 48, stride=2)

    def forward(self, x):
        return self.res2(self.res1(self.in_ds(x)))
'''

_REGRESSER = '''
from torch import nn

from core.extractor import UnetExtractor


class GSRegresser(nn.Module):
    def __init__(self):
        super().__init__()
        self.depth_encoder = UnetExtractor(in_channel=1)
        self.rot_head = nn.Sequential(nn.Conv2d(48, 32, 3, 1, 1), nn.ReLU(), nn.Conv2d(32, 4, 1))
        self.scale_head = nn.Sequential(nn.Conv2d(48, 32, 3, 1, 1), nn.ReLU(), nn.Conv2d(32, 3, 1), nn.Softplus(beta=100))
        self.opacity_head = nn.Sequential(nn.Conv2d(48, 32, 3, 1, 1), nn.ReLU(), nn.Conv2d(32, 1, 1), nn.Sigmoid())

    def forward(self, depth):
        f = self.depth_encoder(depth)
        return self.rot_head(f), self.scale_head(f), self.opacity_head(f)
'''

_PRELUDE = """
import hashlib, json, os, sys
DROPIN, STANDIN = %r, %r
sys.path.insert(0, STANDIN)
sys.path.insert(0, DROPIN)
import torch
from torch import nn
import _bootstrap                                          # what `import corr_sampler` / `import diff_gaussian_rasterization` go through
name = lambda m: type(m).__module__.split(".")[-1] + "." + type(m).__name__


def fresh(value):
    '''The stand-in forgotten, the variable set (None: unset), the drop-in's import path taken.'''
    for m in [m for m in sys.modules if m.split(".")[0] in ("core", "lib")]:
        del sys.modules[m]
    os.environ.pop("GPSGS_ACCELERATE", None)
    if value is not None:
        os.environ["GPSGS_ACCELERATE"] = value
    _bootstrap.submodule("corr")
"""

_MATRIX = """
for value in %r:
    fresh(value)
    A = sys.modules.get("gps_gaussian_amd.accelerate")
    import core.extractor as E, lib.gs_parm_network as G
    torch.manual_seed(11)
    objs = {"unet": E.UnetExtractor(in_channel=3), "block": E.ResidualBlock(32, 48, stride=2),
            "batch": E.ResidualBlock(32, 32, norm="batch").eval(), "net": G.GSRegresser()}
    torch.manual_seed(12)
    with torch.no_grad():
        outs = [objs["unet"](torch.randn(1, 3, 16, 16)), objs["block"](torch.randn(1, 32, 8, 8)), objs["batch"](torch.randn(1, 32, 8, 8)),
                *objs["net"](torch.rand(1, 1, 16, 16))]
    h = hashlib.sha256()
    for o in outs:
        h.update(o.contiguous().numpy().tobytes())
    print("CASE", json.dumps({
        "value": value,
        "installed": sorted(A.installed().items()) if A is not None else [],
        "stems": [[name(m) for m in objs[k].in_ds] for k in ("unet",)] + [[name(m) for m in objs["net"].depth_encoder.in_ds]],
        "norms": {k: [name(m) for m in o.modules() if isinstance(m, nn.GroupNorm)] for k, o in objs.items()},
        "heads": {k: [name(m) for m in getattr(objs["net"], k)][1:] for k in ("rot_head", "scale_head", "opacity_head")},
        "forward": E.ResidualBlock.forward.__module__,
        "calls": dict(A.calls) if A is not None else {},
        "keys": {k: list(o.state_dict().keys()) for k, o in objs.items()},
        "digest": h.hexdigest(),
        "loaded": sorted(m.split(".", 1)[1] for m in sys.modules if m.startswith("gps_gaussian_amd.")),
    }))
    if A is not None:
        A.uninstall()
"""

_CASES = """
ATTRS = [("E", "ResidualBlock", "__init__"), ("E", "ResidualBlock", "forward"), ("E", "UnetExtractor", "__init__"), ("G", "GSRegresser", "__init__")]


def attrs(E, G):
    return [getattr({"E": E, "G": G}[m], c).__dict__[a] for m, c, a in ATTRS]


# ---- restore() and uninstall() put every class attribute back, reset every counter and the conversion state
fresh(None)
import core.extractor as E, lib.gs_parm_network as G       # loaded BEFORE the hook: install() rebinds what is already there
own = attrs(E, G)
os.environ["GPSGS_ACCELERATE"] = "all,groupnorm,resblock,stemconv,gshead"
_bootstrap.submodule("corr")
import gps_gaussian_amd.accelerate as A
assert A._armed and any(type(f).__name__ == "_Finder" for f in sys.meta_path)
assert all(a is not b for a, b in zip(attrs(E, G), own)) and len(A.installed()) == 4 and len(A._originals) == 4
assert [A._originals["%s.%s.%s" % ({"E": "core.extractor", "G": "lib.gs_parm_network"}[m], c, a)][2] for m, c, a in ATTRS] == own
with torch.no_grad():
    G.GSRegresser()(torch.rand(1, 1, 16, 16))
    E.ResidualBlock(32, 32, norm="batch").eval()(torch.randn(1, 32, 8, 8))
assert sum(A.calls.values()) > 0 and all(A.calls[k] > 0 for k in ("resblock", "resblock_passthrough", "groupnorm_passthrough",
                                                                  "stemconv_passthrough", "gshead_passthrough"))
A.restore()
assert all(a is b for a, b in zip(attrs(E, G), own)) and A.installed() == {} and A._originals == {}
assert set(A.calls.values()) == {0}
assert A._armed and any(type(f).__name__ == "_Finder" for f in sys.meta_path)        # restore() undoes the rebinding, not the installation
A.apply(features=("stemconv",))                            # the conversion state is gone: the shared wrapper now converts the stem and nothing else
assert A.installed() == {"core.extractor.UnetExtractor.__init__": "stemconv"}
assert [name(m) for m in E.UnetExtractor().in_ds] == ["stemconv.FusedStemConv2d", "normalization.GroupNorm", "activation.ReLU"]
assert {name(m) for m in G.GSRegresser().modules() if isinstance(m, nn.GroupNorm)} == {"normalization.GroupNorm"}
assert [name(m) for m in G.GSRegresser().rot_head][1:] == ["activation.ReLU", "conv.Conv2d"]
A.uninstall()
assert all(a is b for a, b in zip(attrs(E, G), own)) and A.installed() == {} and A._originals == {} and set(A.calls.values()) == {0}
assert not A._armed and not any(type(f).__name__ == "_Finder" for f in sys.meta_path)
assert [name(m) for m in E.UnetExtractor().in_ds] == ["conv.Conv2d", "normalization.GroupNorm", "activation.ReLU"]
print("OK restore")

# ---- apply(features=...) twice with different names accumulates
fresh(None)
import core.extractor as E, lib.gs_parm_network as G
assert A.apply(features=("groupnorm",)) == 2
assert [name(m) for m in E.UnetExtractor().in_ds] == ["conv.Conv2d", "groupnorm.FusedGroupNorm", "activation.ReLU"]
assert A.apply(features=("stemconv",)) == 0                # the constructor is wrapped already: no new binding, one more conversion
unet = E.UnetExtractor()
assert [name(m) for m in unet.in_ds] == ["stemconv.FusedStemConv2d", "groupnorm.FusedGroupNorm", "activation.ReLU"]
assert {name(m) for m in unet.modules() if isinstance(m, nn.GroupNorm)} == {"groupnorm.FusedGroupNorm"}
assert A.installed() == {"core.extractor.ResidualBlock.__init__": "groupnorm", "core.extractor.UnetExtractor.__init__": "groupnorm"}
assert A.apply(features=("resblock", "gshead")) == 2       # the forward and the heads' constructor on top
assert [name(m) for m in E.UnetExtractor().in_ds] == ["stemconv.FusedStemConv2d", "groupnorm.FusedGroupNormReLU", "linear.Identity"]
assert [name(m) for m in G.GSRegresser().rot_head][1:] == ["linear.Identity", "gshead.FusedHeadConv"]
assert A.installed() == {"core.extractor.ResidualBlock.__init__": "groupnorm", "core.extractor.UnetExtractor.__init__": "groupnorm",
                         "core.extractor.ResidualBlock.forward": "resblock", "lib.gs_parm_network.GSRegresser.__init__": "gshead"}
A.uninstall()
print("OK accumulate")

# ---- late_apply() gives up after 16 tries when a requested module never loads
fresh("loss,groupnorm")                                    # lib.loss does not exist in the stand-in
assert A._armed
walks = []
apply = A.apply
A.apply = lambda *a, **k: (walks.append(1), apply(*a, **k))[1]
try:
    for i in range(15):
        A.late_apply()
    assert A._armed and len(walks) == 15
    A.late_apply()
    assert not A._armed and len(walks) == 16
    for i in range(8):
        A.late_apply()
    assert not A._armed and len(walks) == 16               # a flag test from here on
finally:
    A.apply = apply
import core.extractor as E                                 # the finder still catches a module that loads later
assert A.installed() == {"core.extractor.ResidualBlock.__init__": "groupnorm", "core.extractor.UnetExtractor.__init__": "groupnorm"}
A.uninstall()
# ... and at once when everything requested is in place
fresh(None)
import core.extractor as E
os.environ["GPSGS_ACCELERATE"] = "groupnorm"
_bootstrap.submodule("corr")
assert A._armed and len(A.installed()) == 2
A.late_apply()
assert not A._armed
A.uninstall()
print("OK late_apply")
"""


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """Writes the stand-in package; returns run(body) -> the stdout of a fresh interpreter that ran the prelude and `body`."""
    gps_gaussian_amd.build()                               # the conversions ask the library which configurations it implements
    root = tmp_path_factory.mktemp("standin")
    for pkg, mod, src in (("core", "extractor", _EXTRACTOR), ("lib", "gs_parm_network", _REGRESSER)):
        (root / pkg).mkdir()
        (root / pkg / "__init__.py").write_text("")
        (root / pkg / (mod + ".py")).write_text(src)

    def run(body):
        env = dict(os.environ)
        env.pop("GPSGS_ACCELERATE", None)
        env.pop("GPSGS_ACCELERATE_VERBOSE", None)
        code = textwrap.dedent(_PRELUDE % (gps_gaussian_amd.DROPIN_DIR, str(root))) + textwrap.dedent(body)
        r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env,
                           cwd=str(root))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout
    return run


@pytest.fixture(scope="module")
def matrix(child):
    out = child(_MATRIX % ([_value(c) for c in CASES],))
    recs = [json.loads(l.split(" ", 1)[1]) for l in out.splitlines() if l.startswith("CASE ")]
    assert [r["value"] for r in recs] == [_value(c) for c in CASES]
    return dict(zip(CASES, recs))


@pytest.fixture(scope="module")
def further(child):
    return child(_CASES)


_RB_INIT, _UNET_INIT = "core.extractor.ResidualBlock.__init__", "core.extractor.UnetExtractor.__init__"
_RB_FWD, _GS_INIT = "core.extractor.ResidualBlock.forward", "lib.gs_parm_network.GSRegresser.__init__"
CALL_KEYS = ["pack", "loss", "corr", "upsample", "unproject", "splat", "groupnorm", "resblock", "stemconv", "gshead",
             "loss_passthrough", "unproject_passthrough", "groupnorm_passthrough", "resblock_passthrough", "stemconv_passthrough", "gshead_passthrough"]


def _expected(subset):
    """What the hook's documentation says a subset of the four names does to the stand-in (whether or not `all` is there too: none of the modules
    `all` rebinds exists in it)."""
    gn, rb, sc, gh = (n in subset for n in NAMES)
    installed = []
    if gn or rb:                                           # one wrapper per constructor, filed under groupnorm if both names ask
        installed += [(_RB_INIT, "groupnorm" if gn else "resblock"), (_UNET_INIT, "groupnorm" if gn else "resblock")]
    elif sc:                                               # the stem convolution alone: only the class that has a stem
        installed += [(_UNET_INIT, "stemconv")]
    if rb:
        installed += [(_RB_FWD, "resblock")]
    if gh:
        installed += [(_GS_INIT, "gshead")]
    norm = "groupnorm.FusedGroupNorm" if gn or rb else "normalization.GroupNorm"
    stem = ["stemconv.FusedStemConv2d" if sc else "conv.Conv2d", "groupnorm.FusedGroupNormReLU" if rb else norm,
            "linear.Identity" if rb else "activation.ReLU"]
    # GroupNorm layers in modules() order: the stem's, res1's two, res2's two and the one of its downsample path
    norms = {"unet": [stem[1]] + [norm] * 5, "block": [norm] * 3, "batch": [], "net": [stem[1]] + [norm] * 5}
    tail = ["linear.Identity", "gshead.FusedHeadConv"] if gh else ["activation.ReLU", "conv.Conv2d"]
    heads = {"rot_head": tail, "scale_head": tail + ["linear.Identity" if gh else "activation.Softplus"],
             "opacity_head": tail + ["linear.Identity" if gh else "activation.Sigmoid"]}
    calls = dict.fromkeys(CALL_KEYS, 0)
    if gn or rb:
        calls["groupnorm_passthrough"] = 6 + 3 + 6         # CPU tensors: every converted norm hands its call on, once per norm and forward
    if rb:
        calls["resblock"], calls["resblock_passthrough"] = 2 + 1 + 2, 1     # the GroupNorm blocks on the new forward, the BatchNorm block on its own
    if sc:
        calls["stemconv_passthrough"] = 2                  # the two encoders' stems
    if gh:
        calls["gshead_passthrough"] = 3
    return dict(installed=sorted(installed), stems=[stem, stem], norms=norms, heads=heads, calls=calls,
                forward="gps_gaussian_amd.accelerate" if rb else "core.extractor")


@pytest.mark.parametrize("case", CASES, ids=[_value(c) or "unset" for c in CASES])
def test_every_subset_installs_converts_and_counts_what_it_names(matrix, case):
    rec, want = matrix[case], _expected(case[0])
    assert [tuple(kv) for kv in rec["installed"]] == want["installed"]
    assert rec["stems"] == want["stems"]
    assert rec["norms"] == want["norms"]
    assert rec["heads"] == want["heads"]
    assert rec["forward"] == want["forward"]
    if case == ((), False):                                # the variable unset: the hook is not even imported
        assert rec["calls"] == {} and "accelerate" not in rec["loaded"]
    else:
        assert list(rec["calls"].items()) == list(want["calls"].items())       # every key, in order, with its count
    plain = matrix[((), False)]
    assert rec["keys"] == plain["keys"] and len(plain["keys"]["net"]) > len(plain["keys"]["unet"]) > len(plain["keys"]["block"]) > 0
    assert rec["digest"] == plain["digest"]                # CPU tensors: every converted layer computes with torch's own ops


def test_nothing_is_imported_before_it_is_asked_for(matrix):
    ops = {"groupnorm", "stemconv", "gshead", "splat", "loss", "unproject", "render_api", "pack", "rasterizer"}
    unset, only_all, only_gn = matrix[((), False)], matrix[((), True)], matrix[(("groupnorm",), False)]
    assert "corr" in unset["loaded"] and not (ops | {"accelerate"}) & set(unset["loaded"])
    assert "accelerate" in only_all["loaded"] and not ops & set(only_all["loaded"])
    assert "groupnorm" in only_gn["loaded"] and not (ops - {"groupnorm"}) & set(only_gn["loaded"])


def test_the_counters_and_their_order():
    assert list(A.calls) == CALL_KEYS                      # tools/run_reference.py writes this dict into the reports as it stands


def test_restore_and_uninstall_put_everything_back(further):
    assert "OK restore" in further


def test_apply_accumulates_across_calls(further):
    assert "OK accumulate" in further


def test_late_apply_gives_up_after_16_tries(further):
    assert "OK late_apply" in further
