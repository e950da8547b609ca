"""Opt-in: let the reference's UNMODIFIED scripts reach the fused kernels of SURVEY.md section 8(f).

The two drop-in import names (`diff_gaussian_rasterization`, `corr_sampler`) replace external extensions, so the reference reaches them by
importing.  Everything below replaces code that lives INSIDE the reference, which an unmodified `train_stage2.py` / `test_view_interp.py` never
hands over -- unless asked to:

    GPSGS_ACCELERATE=pack,loss,corr,upsample,unproject   (or "all"; unset / empty = off, the default)

With the variable set, importing either drop-in installs a `sys.meta_path` finder that lets the reference's modules load from where they lie,
untouched, and -- after each one has executed -- rebinds the rows of `_ROWS` to this package: in the defining module and in every loaded module
that had already bound the same object with `from ... import ...` (train_stage2.py:16-17 bind `pts2render`, `l1_loss`, `ssim` after
`lib.network` -> `core.corr` has imported `corr_sampler` at :13, i.e. after this hook is in place).  No reference file changes on disk; nothing
here runs unless the variable is set; every replacement is the GPU path of this package (no CPU fallback).

  name       "all"  what it rebinds or wraps in the reference                                               implemented in
  pack       yes    lib/GaussianRender.py:6-40 `pts2render`                                                 render_api.py
  loss       yes    lib/loss.py:36-83 `l1_loss`, `ssim`                                                     loss.py
  corr       yes    core/corr.py:31-61 `CorrBlockFast1D`                                                    corr.py
  upsample   yes    core/raft_stereo_human.py:69-81 `FlowUpdateModule.upsample_flow`                        corr.py
  unproject  yes    lib/utils.py:88-120 `flow2depth`, `depth2pc`                                            unproject.py
  splat      no     lib/TaichiRender.py, SERVED by the finder instead of executed (`import taichi`,         splat.py
                    `ti.init(ti.cuda)` cannot run on this card): what lets train_stage1.py:16 import it
  groupnorm  no     wraps core/extractor.py:7, :64 `ResidualBlock.__init__`, `UnetExtractor.__init__`:      groupnorm.py
                    after the reference's own constructor every nn.GroupNorm is a FusedGroupNorm
  resblock   no     `groupnorm`, plus core/extractor.py:48 `ResidualBlock.forward` with each norm + ReLU    groupnorm.py
                    and the closing add + ReLU in one op, and the stem's (:66-70) ReLU folded into its norm
  stemconv   no     wraps `UnetExtractor.__init__`: the stem's Conv2d(3 | 1, 32, 5, stride 2, padding 2)    stemconv.py
                    (`in_ds[0]`, core/extractor.py:66-70) becomes a FusedStemConv2d
  gshead     no     wraps lib/gs_parm_network.py:8 `GSRegresser.__init__`: the ReLU -> Conv2d(32, 4|3|1, 1) gshead.py
                    -> nothing | Softplus | Sigmoid tail of its three heads (:34-50) becomes a FusedHeadConv
  conv3x3    no     wraps `GSRegresser.__init__` too: `out_conv` + `out_relu` (:31-32) and the Conv2d(32, 32, 3)   conv3x3.py
                    at the top of each head become FusedConv3x3
  conv1x1    no     wraps `ResidualBlock.__init__`, `UnetExtractor.__init__` too: the Conv2d(in, planes, 1, stride)   conv1x1.py
                    that opens a block's shortcut (`downsample[0]`, core/extractor.py:43-45) becomes a FusedConv1x1

The names outside "all" are accepted by name only (`all,splat`, `resblock,stemconv`, ...) and imply nothing but what their line says; the counters
of the last two (`BY_NAME`, from the table `NAMES`) appear in `calls` when the name is first requested, in the order asked for.  A wrapped
constructor runs the reference's own `__init__` and then the conversions that were asked for (`_ENCODER_STEPS`, `_HEAD_STEPS`): same parameters, same state_dict; the
reference's `forward` bodies run as they are, `resblock`'s one rebinding apart.  Instances are built long after import, so the import order of
these modules against the drop-in does not matter.  One wrapper per constructor serves every name that asks for it and does only what was asked:
`stemconv` alone leaves every norm an `nn.GroupNorm` (and ResidualBlock, which has no stem, unwrapped), `groupnorm` alone leaves `in_ds[0]` a
plain `nn.Conv2d`, `gshead` touches the heads and nothing else, `conv1x1` changes `downsample[0]` and leaves `downsample[1]` to `groupnorm`.

`installed()` reports what was rebound, `calls` counts how often each replacement ran (the tests assert the kernels were reached).
"""
import importlib
import importlib.abc
import importlib.util
import os
import sys
import threading

# Every name GPSGS_ACCELERATE accepts, in the order requested() answers in: name -> (implied by "all", has a <name>_passthrough counter, its
# counters exist from import).  A passthrough counter counts the calls that went THROUGH a replacement but were handed on to the reference's or
# torch's own code (a configuration the fused kernel does not implement: ssim with another window, CPU tensors, channels-last, norm_fn batch, ...),
# so that a run on the eager path for those calls leaves a trace; the full-pipeline runner prints them.  The counters of a
# name whose last column is False are created in `calls` when the name is first requested or first counted (counters()), behind every existing
# key, so a process that never asks for one keeps the keys of the other names, in their order.  Everything below is derived from this table.
NAMES = {
    "pack":      (True,  False, True),
    "loss":      (True,  True,  True),
    "corr":      (True,  False, True),
    "upsample":  (True,  False, True),
    "unproject": (True,  True,  True),
    "splat":     (False, False, True),
    "groupnorm": (False, True,  True),
    "resblock":  (False, True,  True),
    "stemconv":  (False, True,  True),
    "gshead":    (False, True,  True),
    "conv3x3":   (False, True,  False),
    "conv1x1":   (False, True,  False),
}
FEATURES = tuple(n for n, row in NAMES.items() if row[0])                       # what "all" means
OPT_IN = tuple(n for n, row in NAMES.items() if not row[0] and row[2])          # accepted by name only, never implied by "all"
BY_NAME = tuple(n for n, row in NAMES.items() if not row[0] and not row[2])     # by name only as well; counters on first request
_PREFIXES = ("lib", "core", "gaussian_renderer", "config", "train_stage1", "train_stage2", "test_view_interp", "test_real_data")
_SUBSTITUTES = {"lib.TaichiRender": "splat"}   # module served instead of the reference's file -> the opt-in name that asks for it


def _keys(*names):
    """The counters of `names`: one per name, then the <name>_passthrough of those that have one."""
    return names + tuple(n + "_passthrough" for n in names if NAMES[n][1])


calls = dict.fromkeys(_keys(*FEATURES, *OPT_IN), 0)
_asked = set()           # the opt-in names apply() has been given so far: what the constructor wrappers convert (_ENCODER_STEPS, _HEAD_STEPS)
_installed = {}          # "module.attr" -> feature
_originals = {}          # "module.attr" -> (holder, name, the reference's own object): restore(), original(), and the two pass-through cases below
_armed = False           # set by install(); cleared once every requested name is rebound (late_apply() is then a flag test)
_lock = threading.RLock()
_finder = None


def requested(value=None):
    """The feature set GPSGS_ACCELERATE asks for (an unknown name raises: a typo must not silently run the eager path)."""
    v = os.environ.get("GPSGS_ACCELERATE", "") if value is None else value
    v = v.strip().lower()
    if v in ("", "0", "off", "none", "false"):
        return ()
    if v in ("1", "all", "on", "true"):
        return FEATURES
    names = tuple(x.strip() for x in v.replace(";", ",").split(",") if x.strip())
    if any(x in ("1", "all", "on", "true") for x in names):
        names += FEATURES
    known = tuple(NAMES)
    bad = [x for x in names if x not in known + ("1", "all", "on", "true")]
    if bad:
        raise ValueError("GPSGS_ACCELERATE: unknown feature(s) %s (known: %s)" % (bad, ", ".join(known)))
    for f in BY_NAME:
        if f in names:
            counters(f)
    return tuple(f for f in known if f in names)


def counters(name):
    """`calls`, with the counters of the BY_NAME feature `name` in it (created at zero, behind every existing key, the first time)."""
    if name not in calls:
        with _lock:
            for k in _keys(name):
                calls.setdefault(k, 0)
    return calls


def installed():
    return dict(_installed)


def original(obj, name):
    """The reference's own attribute `name` that was rebound on the class of `obj` (or on a base of it); None if none was."""
    for holder, n, orig in list(_originals.values()):
        if n == name and isinstance(holder, type) and isinstance(obj, holder):
            return orig
    return None


# ---- the replacements (thin: argument shapes of the reference on the outside, this package's fused ops inside) -------------------------
def _pts2render(data, bg_color):
    """lib/GaussianRender.py:6 -- same contract; fused pack + one autograd node for the batch (render_api.pts2render)."""
    from . import render_api
    calls["pack"] += 1
    return render_api.pts2render(data, bg_color)


def _l1_loss(network_output, gt):
    from . import loss
    calls["loss"] += 1
    return loss.l1_and_ssim_shared(network_output, gt)[0]


def _ssim(img1, img2, window_size=11, size_average=True):
    from . import loss
    if window_size != 11 or not size_average:
        # not the configuration the fused kernel implements: the reference's own function (still on the GPU, still the reference's code)
        calls["loss_passthrough"] += 1
        return _originals["lib.loss.ssim"][2](img1, img2, window_size, size_average)
    calls["loss"] += 1
    return loss.l1_and_ssim_shared(img1, img2)[1]


def _upsample_flow(self, flow, mask):
    """core/raft_stereo_human.py:69 (a method of FlowUpdateModule)."""
    from . import corr
    calls["upsample"] += 1
    return corr.upsample_flow(flow, mask, 2 ** self.args.n_downsample)


def _flow2depth(data):
    """lib/utils.py:113 -- returns the inverse-depth map; the SAME launch also produced the world points, which ride on the returned tensor
    until lib/network.py:67 asks for them through depth2pc (the reference calls the two back to back, lib/network.py:66-67)."""
    from . import unproject
    calls["unproject"] += 1
    depth, xyz, _valid = unproject.unproject(data['flow_pred'], data['mask'], data['ref_intr'], data['intr'], data['extr'], data['Tf_x'])
    depth._gpsgs_xyz = (xyz, data['extr'], data['intr'])
    return depth


def _depth2pc(depth, extrinsic, intrinsic):
    """lib/utils.py:88 -- the points computed together with `depth` when it came from _flow2depth with these cameras; any other depth map goes
    through the reference's own function."""
    stash = getattr(depth, "_gpsgs_xyz", None)
    if stash is not None and stash[1] is extrinsic and stash[2] is intrinsic:
        return stash[0]
    calls["unproject_passthrough"] += 1
    return _originals["lib.utils.depth2pc"][2](depth, extrinsic, intrinsic)


# what a wrapped constructor runs on the new instance, in this order: (the names that ask for the step, module of this package, function)
_ENCODER_STEPS = ((("groupnorm", "resblock"), "groupnorm", "convert"),             # nn.GroupNorm -> FusedGroupNorm
                  (("resblock",), "groupnorm", "fuse_sequential_relu"),            # the stem's ReLU folded into its norm
                  (("stemconv",), "stemconv", "convert"),                          # the stem convolution
                  (("conv1x1",), "conv1x1", "convert"))                            # the 1x1 convolution that opens a block's shortcut
# the heads' tails and nothing else: the encoder and the blocks GSRegresser builds went through their own wrappers inside its constructor
_HEAD_STEPS = ((("gshead",), "gshead", "convert"),
               (("conv3x3",), "conv3x3", "convert_regresser"))                     # out_conv + out_relu, and the 3x3 layer that opens each head


def _converting_init(key, steps):
    """The reference's own constructor (from _originals), then the steps whose names were asked for."""
    def __init__(self, *args, **kwargs):
        _originals[key][2](self, *args, **kwargs)
        for names, module, function in steps:
            if not _asked.isdisjoint(names):
                getattr(importlib.import_module("." + module, __package__), function)(self)
    return __init__


_resblock_init = _converting_init("core.extractor.ResidualBlock.__init__", _ENCODER_STEPS)      # core/extractor.py:7
_unet_init = _converting_init("core.extractor.UnetExtractor.__init__", _ENCODER_STEPS)          # core/extractor.py:64
_regresser_init = _converting_init("lib.gs_parm_network.GSRegresser.__init__", _HEAD_STEPS)     # lib/gs_parm_network.py:8


def _resblock_forward(self, x):
    """core/extractor.py:48 -- the block on the fused norm + ReLU (+ add + ReLU) ops; blocks without GroupNorm run the reference's forward."""
    from . import groupnorm
    return groupnorm.residual_block_forward(self, x)


_corr_cls = None


def _corr_block():
    """core/corr.py:31 -- this package's CorrBlockFast1D (fused volume + pyramid build, all levels sampled in one launch), counting its uses."""
    global _corr_cls
    if _corr_cls is None:
        from . import corr

        class CorrBlockFast1D(corr.CorrBlockFast1D):
            def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
                calls["corr"] += 1
                super().__init__(fmap1, fmap2, num_levels=num_levels, radius=radius)

        _corr_cls = CorrBlockFast1D
    return _corr_cls


_FACTORIES = (_corr_block,)   # replacements made on first use (they import their op module): called with no argument for the object to bind

# (defining module, attribute or 'Class.attr', replacement, the names that ask for the row).  A row is filed -- in _table(), installed() -- under
# the first REQUESTED name of its list: one wrapper per constructor, whichever name asks (`groupnorm` and `resblock`: filed under `groupnorm`;
# `stemconv` alone: only the class that has a stem)
_ROWS = (
    ("lib.GaussianRender", "pts2render", _pts2render, ("pack",)),
    ("lib.loss", "l1_loss", _l1_loss, ("loss",)),
    ("lib.loss", "ssim", _ssim, ("loss",)),
    ("core.corr", "CorrBlockFast1D", _corr_block, ("corr",)),
    ("core.raft_stereo_human", "FlowUpdateModule.upsample_flow", _upsample_flow, ("upsample",)),
    ("lib.utils", "flow2depth", _flow2depth, ("unproject",)),
    ("lib.utils", "depth2pc", _depth2pc, ("unproject",)),
    ("core.extractor", "ResidualBlock.__init__", _resblock_init, ("groupnorm", "resblock", "conv1x1")),
    ("core.extractor", "UnetExtractor.__init__", _unet_init, ("groupnorm", "resblock", "stemconv", "conv1x1")),
    ("lib.gs_parm_network", "GSRegresser.__init__", _regresser_init, ("gshead", "conv3x3")),
    ("core.extractor", "ResidualBlock.forward", _resblock_forward, ("resblock",)),
)


def _table(features):
    """feature -> [(defining module, attribute or 'Class.attr', replacement)], with an entry for every requested feature."""
    t = {f: [] for f in features}
    for modname, attr, repl, names in _ROWS:
        feat = next((n for n in names if n in t), None)
        if feat is not None:
            t[feat].append((modname, attr, repl() if repl in _FACTORIES else repl))
    return t


def _loaded(name):
    """A module that has finished executing (a module still inside its own import is in sys.modules too)."""
    m = sys.modules.get(name)
    if m is None:
        return None
    spec = getattr(m, "__spec__", None)
    if spec is not None and getattr(spec, "_initializing", False):
        return None
    return m


def apply(features=None):
    """Rebind whatever can be rebound NOW (idempotent; called after every reference module finishes loading).  Returns the number of new
    bindings made."""
    feats = requested() if features is None else tuple(features)
    if not feats:
        return 0
    made = 0
    with _lock:
        _asked.update(f for f in feats if f in OPT_IN + BY_NAME)
        for feat, rows in _table(feats).items():
            for modname, attr, repl in rows:
                mod = _loaded(modname)
                if mod is None:
                    continue
                key = modname + "." + attr
                holder, name = mod, attr
                if "." in attr:
                    cls, name = attr.split(".")
                    holder = getattr(mod, cls, None)
                    if holder is None:
                        continue
                cur = holder.__dict__.get(name) if isinstance(holder, type) else getattr(holder, name, None)
                if cur is None or cur is repl:
                    continue
                if key not in _originals:
                    _originals[key] = (holder, name, cur)
                orig = _originals[key][2]
                setattr(holder, name, repl)
                if _installed.get(key) is None:
                    _installed[key] = feat
                    made += 1
                if holder is mod:
                    # names other loaded modules bound with `from <modname> import <attr>` before this ran (also `__main__`)
                    for other in list(sys.modules.values()):
                        d = getattr(other, "__dict__", None)
                        if d is not None and other is not mod and d.get(name) is orig:
                            d[name] = repl
                            _installed["%s.%s" % (getattr(other, "__name__", "?"), name)] = feat
    if made and os.environ.get("GPSGS_ACCELERATE_VERBOSE"):
        print("[gps_gaussian_amd.accelerate] rebound: " + ", ".join(sorted(_installed)), file=sys.stderr)
    return made


def restore():
    """Undo every rebinding (tests)."""
    with _lock:
        for key, (holder, name, orig) in list(_originals.items()):
            repl = holder.__dict__.get(name) if isinstance(holder, type) else getattr(holder, name, None)
            setattr(holder, name, orig)
            if not isinstance(holder, type) and repl is not None:
                for other in list(sys.modules.values()):
                    d = getattr(other, "__dict__", None)
                    if d is not None and d.get(name) is repl:
                        d[name] = orig
        _originals.clear()
        _installed.clear()
        _asked.clear()
        for k in _keys(*BY_NAME):              # back to the keys a process starts with
            calls.pop(k, None)
        for k in calls:
            calls[k] = 0


_late_calls = 0


def late_apply():
    """Safety net for import orders in which no reference module loads after the drop-in (nothing for the finder to hook): the shims call this
    on first use.  A flag test once everything requested is in place -- or after 16 tries: a requested feature whose module the script never imports
    (`loss` in a pure inference script that does not touch lib.loss) must not cost every later render call a table walk; the finder still catches
    the module should it load later."""
    global _armed, _late_calls
    if not _armed:
        return
    apply()
    _late_calls += 1
    feats = requested()
    want = sum(len(rows) for rows in _table(feats).values())
    if len(_originals) >= want or _late_calls >= 16:
        _armed = False


class _AfterExec(importlib.abc.Loader):
    """Delegates to the module's real loader (source or sourceless), then gives apply() a chance."""

    def __init__(self, real):
        self._real = real

    def create_module(self, spec):
        return self._real.create_module(spec)

    def exec_module(self, module):
        self._real.exec_module(module)
        spec = getattr(module, "__spec__", None)
        init = getattr(spec, "_initializing", None)
        try:
            if init:
                spec._initializing = False   # the body HAS run; the import machinery clears the flag only after we return
            apply()
        finally:
            if init:
                spec._initializing = init

    def __getattr__(self, name):   # get_code / get_source / is_package / get_filename ... of the real loader (runpy, inspect, linecache)
        return getattr(self._real, name)


class _Substitute(importlib.abc.Loader):
    """Loads this package's stand-in for a reference module that cannot execute here (lib.TaichiRender: `import taichi`)."""

    def __init__(self, feature):
        self.feature = feature

    def create_module(self, spec):
        return None

    def exec_module(self, module):
        from . import splat
        module.TaichiRenderBatch = splat.TaichiRenderBatch
        with _lock:
            _installed[module.__name__ + ".TaichiRenderBatch"] = self.feature


class _Finder(importlib.abc.MetaPathFinder):
    """Finds the reference's modules with the ordinary finders and wraps their loader; every other import passes through untouched."""

    def find_spec(self, name, path=None, target=None):
        if name.split(".", 1)[0] not in _PREFIXES:
            return None
        feat = _SUBSTITUTES.get(name)
        if feat is not None and feat in requested():
            return importlib.util.spec_from_loader(name, _Substitute(feat), origin="gps_gaussian_amd.accelerate")
        for f in sys.meta_path:
            if f is self or not hasattr(f, "find_spec"):
                continue
            spec = f.find_spec(name, path, target)
            if spec is not None:
                if spec.loader is not None and hasattr(spec.loader, "exec_module") and not isinstance(spec.loader, _AfterExec):
                    spec.loader = _AfterExec(spec.loader)
                return spec
        return None


def install():
    """Called by the drop-in shims on import.  Off (a no-op) unless GPSGS_ACCELERATE names features."""
    global _finder, _armed
    feats = requested()
    if not feats:
        return ()
    with _lock:
        if _finder is None:
            _finder = _Finder()
            sys.meta_path.insert(0, _finder)
        _armed = True
    apply(feats)
    return feats


def uninstall():
    global _finder, _armed, _late_calls
    with _lock:
        _armed = False
        _late_calls = 0
        if _finder is not None and _finder in sys.meta_path:
            sys.meta_path.remove(_finder)
        _finder = None
    restore()
