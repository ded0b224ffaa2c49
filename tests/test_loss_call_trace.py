"""The loss layer's launch sequence, pinned on the CPU.

``dvf.lib.lib`` is replaced by an object whose every attribute records ``(symbol, args)`` and returns 0 (a small size for the
``*_floats`` queries), ``dvf.lib.dev`` / ``ptr_array`` by functions that name a pointer instead of checking it, so the whole
loss layer -- loss_functions*.py, the five step bodies of dvf/steps.py and the autograd Functions of dvf/ops.py -- runs
forward and backward on CPU tensors without a kernel.  A TorchDispatchMode interleaves the aten operators that would launch
one.  The networks are stubs that return leaf tensors.

tests/loss_call_traces.json holds the traces of the commit BEFORE the photometric appearance term moved into
dvf/appearance.py (``python tests/test_loss_call_trace.py --record`` wrote it there).  For every case the C-ABI calls, scalar
arguments included, must come in exactly that order, and the aten operators must be a sub-multiset of the recorded ones: a
change of the Python layer may drop an unused copy, never add a launch or reorder the kernels.  In deterministic mode the
same calls with the same arguments in the same order are the same bits."""
import collections
import json
import os
import sys

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

TRACES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "loss_call_traces.json")

# aten operators that launch nothing: allocations (the caching allocator) and views
NO_LAUNCH = {
    "empty.memory_format", "empty_like.default", "empty_strided.default", "new_empty.default", "new_empty_strided.default",
    "view.default", "_unsafe_view.default", "_reshape_alias.default", "reshape.default", "select.int", "slice.Tensor",
    "unsqueeze.default", "squeeze.dim", "squeeze.default", "squeeze.dims", "transpose.int", "t.default", "permute.default",
    "expand.default", "as_strided.default", "detach.default", "alias.default", "unbind.int", "split.Tensor",
    "split_with_sizes.default", "lift_fresh.default", "view_as.default",
}


class _Ptr:
    """What the stubbed ``dev`` returns: a name and a byte offset (SsimL1LossFn adds one to its mask pointer)."""

    def __init__(self, name, off=0):
        self.name, self.off = name, off

    def __add__(self, n):
        return _Ptr(self.name, self.off + int(n))

    def token(self):
        return self.name if self.off == 0 else f"{self.name}+{self.off}"


class _Recorder(TorchDispatchMode):
    """One list of events in program order: ``[symbol, [args]]`` for a C-ABI call, ``"aten.<op>"`` for an aten operator."""

    def __init__(self):
        super().__init__()
        self.events = []
        self.names = {}              # data_ptr -> registered name
        self.keep = []               # the registered tensors stay alive, so no later allocation takes a registered address
        self.made = set()            # data_ptr of every tensor an operator returned under the mode
        self.paused = False          # True while a stub builds its inputs: those operators are not the loss layer's

    def register(self, name, t):
        self.names[t.data_ptr()] = name
        self.keep.append(t)
        return t

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func.__name__ if hasattr(func, "__name__") else str(func)
        if name not in NO_LAUNCH and not self.paused:
            self.events.append("aten." + name)
        out = func(*args, **(kwargs or {}))
        self.made.update(t.data_ptr() for t in (out if isinstance(out, (tuple, list)) else [out]) if torch.is_tensor(t))
        return out

    # ---- the stubs
    def dev(self, t, name="tensor"):
        return None if t is None else _Ptr(self.names.get(t.data_ptr(), "p"))

    def ptr_array(self, tensors, name="tensors"):
        return tuple(self.dev(t) for t in tensors)

    def _arg(self, a):
        if a is None or isinstance(a, (float, str)):
            return a
        if isinstance(a, _Ptr):
            return a.token()
        if isinstance(a, tuple):
            return [self._arg(x) for x in a]
        if isinstance(a, int):
            # (MinReprojLossFn hands select.data_ptr() / counts.data_ptr() to the ABI as raw addresses)
            return self.names.get(a, "p") if a in self.made or a in self.names else a
        raise TypeError(f"unexpected C-ABI argument {a!r}")

    def __getattr__(self, symbol):
        if not symbol.startswith("dvf_"):
            raise AttributeError(symbol)

        def call(*args):
            self.events.append([symbol, [self._arg(a) for a in args]])
            return 8 if symbol.endswith("_floats") else 0
        return call


def _install(monkeypatch):
    import dvf.lib as L
    import dvf.steps as steps
    r = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: r)
    monkeypatch.setattr(L, "dev", r.dev)
    monkeypatch.setattr(L, "ptr_array", r.ptr_array)
    monkeypatch.setattr(L, "stream", lambda: None)
    monkeypatch.setattr(L, "stream_raw", lambda: None)
    monkeypatch.setattr(steps, "POSE_STREAM", False)
    return r


@pytest.fixture
def rec(monkeypatch):
    return _install(monkeypatch)


# ------------------------------------------------------------------------------------------------ inputs and stub networks

B, H, W = 2, 32, 64


def _leaf(r, name, *shape, grad=True):
    r.paused = True
    t = (torch.rand(*shape, generator=torch.Generator().manual_seed(len(r.names))) + 0.5).requires_grad_(grad)
    r.paused = False
    return r.register(name, t)


def _batch(r, n_views=2):
    from dvf.synthetic import synthetic_batch
    r.paused = True
    batch = synthetic_batch(B, H, W, seed=1234, n_views=n_views)
    r.paused = False
    for k, v in batch.items():
        for i, t in enumerate(v if isinstance(v, list) else [v]):
            r.register(f"{k}{i}" if isinstance(v, list) else k, t)
    return batch


def _depth_net(r, scales=4):
    return lambda img: [_leaf(r, f"disp{s}", B, 1, H >> s, W >> s) for s in range(scales)]


def _pose_net(r):
    return lambda frames: (None, _leaf(r, "pose", B, 6))


class _PoseExpStub:
    def __init__(self, r, nb_ref_imgs=2, masks=True):
        self.r, self.nb_ref_imgs, self.masks = r, nb_ref_imgs, masks

    def __call__(self, tgt, refs):
        assert len(refs) == self.nb_ref_imgs
        v = self.nb_ref_imgs
        masks = [_leaf(self.r, f"mask{s}", B, v, H >> s, W >> s) if self.masks else None for s in range(4)]
        return masks, _leaf(self.r, "pose", B, v, 6)


def _feat_net(r):
    return lambda x: _leaf(r, "feat", x.size(0), 32, x.size(2), x.size(3))


class _FrozenFeat:
    """paper_losses runs its extractor under no_grad: the maps it returns carry no graph."""

    def __init__(self, r):
        self.r = r

    def __call__(self, x):
        assert not torch.is_grad_enabled()
        return _leaf(self.r, "feat", x.size(0), 32, x.size(2), x.size(3), grad=False)


# --------------------------------------------------------------------------------------------------------------- the cases

_MODES = {"l1": {}, "ssim": dict(ssim_weight=0.85), "minreproj": dict(ssim_weight=0.85, min_reprojection=True, auto_mask=True)}


def _lf(mode):
    def run(r):
        import loss_functions as LF
        b = _batch(r)
        depth, t21 = _leaf(r, "depth", B, H, W), _leaf(r, "pose", B, 6)
        counts = []
        loss = LF.photometric_reconstruction_loss(b["img_R2"], b["img_R1"], b["img_L2"], depth, t21, b["T_R2L"], b["K"], b["Kinv"],
                                                  img_scale=0.004, selection_counts=counts, **_MODES[mode])
        assert len(counts) == (1 if mode == "minreproj" else 0)
        return loss
    return run


def _ls(mode):
    def run(r):
        import loss_functions_sfm as LS
        b = _batch(r)
        depth = [_leaf(r, f"depth{s}", B, 1, H >> s, W >> s) for s in range(2)]
        masks = [None, None] if mode == "minreproj" else [_leaf(r, f"mask{s}", B, 2, H >> s, W >> s) for s in range(2)]
        counts = []
        loss = LS.photometric_reconstruction_loss(b["img_R2"], [b["img_R1"], b["img_L2"]], b["K"], b["Kinv"], depth, masks,
                                                  _leaf(r, "pose", B, 2, 6), selection_counts=counts, **_MODES[mode])
        assert len(counts) == (2 if mode == "minreproj" else 0)
        return loss
    return run


def _abs_warp(r):
    import loss_functions_caffe as LC
    b = _batch(r)
    return LC.abs_warp_loss(b["img_R2"], (b["img_L2"], b["img_R1"]), _leaf(r, "depth", B, 1, H, W),
                            (b["T_R2L_se3"], _leaf(r, "pose", B, 6)), b["K"], b["Kinv"], img_scale=0.004)


def _unsupervise(feat=False, **kw):
    def run(r):
        from dvf.steps import unsupervise_losses
        loss, terms = unsupervise_losses(_depth_net(r), _pose_net(r), _batch(r), feat_extractor=_feat_net(r) if feat else None, **kw)
        assert set(terms) == {"img", "smooth", "total"} | ({"feat"} if feat else set()) | ({"automask"} if kw.get("auto_mask") else set())
        return loss
    return run


def _train_sfm(feat=False, nb_ref_imgs=2, masks=True, **kw):
    def run(r):
        from dvf.steps import train_sfm_losses
        loss, terms = train_sfm_losses(_depth_net(r), _PoseExpStub(r, nb_ref_imgs, masks), _batch(r, nb_ref_imgs),
                                       feat_extractor=_feat_net(r) if feat else None, **kw)
        assert set(terms) == ({"photo", "smooth", "lr", "total"} | ({"feat"} if feat else set()) |
                              ({"automask"} if kw.get("auto_mask") else set()) | ({"exp"} if kw.get("w2", 0) > 0 else set()))
        return loss
    return run


def _depth_only(r):
    from dvf.steps import depth_only_losses
    loss, terms = depth_only_losses(_depth_net(r), _batch(r))
    assert set(terms) == {"img", "smooth", "total"}
    return loss


def _dvo(**kw):
    def run(r):
        from dvf.steps import unsupervise_dvo_losses
        loss, terms = unsupervise_dvo_losses(_depth_net(r), _pose_net(r), _batch(r), **kw)
        assert set(terms) == {"photo", "smooth", "total"}
        return loss
    return run


def _paper(feat):
    def run(r):
        from dvf.steps import paper_losses
        loss, terms = paper_losses(_depth_net(r), _pose_net(r), _batch(r), feat_extractor=_FrozenFeat(r) if feat else None)
        assert set(terms) == {"photo", "smooth", "total"} | ({"feat"} if feat else set())
        return loss
    return run


_RECIPE = dict(ssim_weight=0.85, min_reprojection=True, auto_mask=True, full_res_multiscale=True)   # tests/test_gpu_normsmooth.py

CASES = {
    "lf-l1": _lf("l1"), "lf-ssim": _lf("ssim"), "lf-minreproj": _lf("minreproj"),
    "ls-l1": _ls("l1"), "ls-ssim": _ls("ssim"), "ls-minreproj": _ls("minreproj"),
    "abs-warp": _abs_warp,
    "unsupervise": _unsupervise(),
    "unsupervise-feat": _unsupervise(feat=True),
    "unsupervise-minreproj-ssim": _unsupervise(ssim_weight=0.85, min_reprojection=True, auto_mask=True),
    "unsupervise-ssim-feat": _unsupervise(feat=True, ssim_weight=0.85),
    "unsupervise-normsmooth": _unsupervise(normalized_smoothness=True),
    "sfm-w2": _train_sfm(w2=0.2),
    "sfm-ssim": _train_sfm(w2=0.2, ssim_weight=0.85),
    "sfm-minreproj": _train_sfm(masks=False, min_reprojection=True, auto_mask=True),
    "sfm-fullres-masks": _train_sfm(w2=0.2, full_res_multiscale=True),
    "sfm-recipe-normsmooth": _train_sfm(masks=False, normalized_smoothness=True, **_RECIPE),
    "sfm-recipe-normsmooth-feat": _train_sfm(feat=True, masks=False, normalized_smoothness=True, **_RECIPE),
    "sfm-feat": _train_sfm(feat=True, w2=0.2),
    "sfm-4refs": _train_sfm(nb_ref_imgs=4, w2=0.2),
    "sfm-4refs-ssim": _train_sfm(nb_ref_imgs=4, w2=0.2, ssim_weight=0.85),
    "depth-only": _depth_only,
    "dvo": _dvo(), "dvo-normsmooth": _dvo(normalized_smoothness=True),
    "paper": _paper(False), "paper-frozen-feat": _paper(True),
}


def _trace(r, case):
    with r:
        CASES[case](r).backward()
    return r.events


def _abi(events):
    return [e for e in events if not isinstance(e, str)]


def _aten(events):
    return collections.Counter(e for e in events if isinstance(e, str))


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_sequence_is_the_recorded_one(rec, case):
    with open(TRACES) as f:
        want = json.load(f)[case]
    got = json.loads(json.dumps(_trace(rec, case)))           # tuples -> lists, floats through the same text form
    assert len(_abi(got)) > 0
    for i, (g, w) in enumerate(zip(_abi(got), _abi(want))):
        assert g == w, f"C-ABI call {i}: got {g}, recorded {w}"
    assert len(_abi(got)) == len(_abi(want))
    extra = _aten(got) - _aten(want)
    assert not extra, f"aten operators the recorded trace does not have: {dict(extra)}"


def test_every_recorded_case_is_run():
    with open(TRACES) as f:
        assert sorted(json.load(f)) == sorted(CASES)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_loss_call_trace.py --record   (rewrites loss_call_traces.json from the checked-out code)")
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), os.path.join(os.path.dirname(here), "depth-vo-feat_amd")]
    mp = pytest.MonkeyPatch()
    out = {}
    for name in sorted(CASES):
        out[name] = _trace(_install(mp), name)
        mp.undo()
    with open(TRACES, "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in out.items()) + "\n}\n")
    print({k: len(_abi(v)) for k, v in out.items()})
