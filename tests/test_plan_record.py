"""The convolution plan record (dvf_conv2d_last_plans) is named once per side: the table and constants of include/dvf_hip.h
and dvf.lib.PlanRecord must agree, one hand-written record per kernel family decodes to the fields its call site wrote, a
record stays the plain tuple it always was, and a name of another family raises.  No GPU and no library call."""
import os
import re

import pytest

from conftest import ROOT
from dvf import conv as C
from dvf import lib as L

HEADER = open(os.path.join(ROOT, "include", "dvf_hip.h")).read()

# one record per family as the call sites of csrc/ write it: (op, kernel, 11 ints) -> the fields it must decode to
SAMPLES = {
    "conv_pipe": (("fwd", 1, 2, 1, 1, 16, 3, 4, 1, 3, 512, 77824, 2 | 4 << 4 | 1 << 8 | 0 << 9 | 1 << 10 | 12 << 11),
                  dict(MT=2, NT=1, WM=1, CK=16, TBU=3, KS=4, BN=1, NST=3, threads=512, lds=77824, out_mode="ws", ncls=4, x4=True,
                       blocked=False, lr=True, npi=12)),
    "conv_gather": (("dgrad", 2, 1, 2, 1, 8, 0, 2, 1, 1, 256, 9216, 1 | 4 << 4),
                    dict(MT=1, NT=2, WM=1, CK=8, TBU=0, KS=2, BN=1, NST=1, threads=256, lds=9216, out_mode="atomic", ncls=4)),
    "head_fwd": (("fwd", 3, 2, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0), dict(C_out=2, nseg=3)),
    "head_dgrad": (("dgrad", 4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), dict(C_out=4)),
    "head_wgrad": (("wgrad", 5, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0), dict(C_out=1, ordered=1)),
    "conv_wgrad": (("wgrad", 6, 2, 1, 1, 8, 4, 6, 1, 2, 256, 30720, 49),
                   dict(MT=2, NTW=1, prefetch=1, CK=8, BH=4, PSPLIT=6, vec_p=1, stride=2, threads=256, lds=30720, taps=49,
                        ordered=False)),
    "head_seg_dgrad": (("dgrad", 7, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), dict(segc=16)),
    "wgrad_pipe": (("wgrad", 8, 2 | 32 << 8, 3, 1 | 2, 8, 1, 5, 256, 65536, 9, 136, 2),
                   dict(MT=2, TILE=32, NTW=3, x4=True, ordered=True, CK=8, stride=1, pieces=5, blocks=256, lds=65536, taps=9,
                        row_stride=136, nseg=2)),
    "dconvt_fwd": (("fwd", 9, 16, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0), dict(C_out=16, KH=4)),
}
ALL = sorted(SAMPLES)


def test_header_and_python_agree():
    enum = dict((n, int(v)) for n, v in re.findall(r"\bDVF_K_(\w+) = (\d+)", HEADER))
    assert len(enum) == 9 and {v: n for n, v in enum.items()}.keys() == L.KERNELS.keys()
    for name, value in enum.items():
        assert getattr(L, "K_" + name) == value, name
    assert sorted(L.KERNELS.values()) == ALL
    # DVF_PLAN_INTS, DVF_PLAN_MAX and every shift / mask of the packed words
    defines = dict((n, int(v)) for n, v in re.findall(r"#define DVF_(PLAN_\w+) (\d+)", HEADER))
    assert len(defines) == 13, defines
    for name, value in defines.items():
        assert getattr(L, name) == value, name
    assert {n for n in vars(L) if re.fullmatch(r"PLAN_\w+_(SHIFT|MASK)", n)} == set(defines) - {"PLAN_INTS", "PLAN_MAX"}
    for k in L.KERNELS:
        assert len(L.PLAN_FIELDS[k]) <= L.PLAN_INTS - 1 and len(set(L.PLAN_FIELDS[k])) == len(L.PLAN_FIELDS[k]), k
        for word, shift, mask, conv in L.PLAN_PACKED.get(k, {}).values():
            assert word in L.PLAN_FIELDS[k], (k, word)
    assert set(L.PLAN_FIELDS) == set(L.KERNELS) and set(L.PLAN_PACKED) <= set(L.KERNELS)


def test_header_table_names_every_field():
    """The comment above dvf_conv2d_last_plans lists each family with its field names in PLAN_FIELDS order."""
    table = HEADER[HEADER.index("Which kernels the LAST"):HEADER.index("enum { DVF_K_PIPE")]
    for k, name in L.KERNELS.items():
        line = re.search(r"^ \*   %s +(.*)$" % name, table, re.M).group(1)
        listed = tuple(w.split()[0] for w in re.sub(r"\(.*?\)", "", line).split(","))
        assert listed == L.PLAN_FIELDS[k], (name, listed)


@pytest.mark.parametrize("family", ALL)
def test_sample_decodes(family):
    t, want = SAMPLES[family]
    assert len(t) == 1 + L.PLAN_INTS
    r = L.PlanRecord(t)
    assert (r.op, r.kernel, r.kernel_name) == (t[0], t[1], family)
    got = {name: getattr(r, name) for name in want}
    assert got == want and all(type(got[n]) is type(want[n]) for n in want), got
    # nothing else is readable: the names are exactly the family's fields and packed sub-fields
    names = set(L.PLAN_FIELDS[r.kernel]) | set(L.PLAN_PACKED.get(r.kernel, ()))
    assert set(want) == names - {"flags", "tile", "lanes"}, names
    for word in names & {"flags", "tile", "lanes"}:
        assert getattr(r, word) == t[2 + L.PLAN_FIELDS[r.kernel].index(word)]


@pytest.mark.parametrize("family", ALL)
def test_record_is_the_plain_tuple(family):
    t = SAMPLES[family][0]
    r = L.PlanRecord(t)
    assert r == t and t == r and hash(r) == hash(t) and tuple(r) == t
    assert r in {t} and t in {r} and len({r, t}) == 1
    other = SAMPLES["dconvt_fwd" if family != "dconvt_fwd" else "head_fwd"][0]
    assert sorted([r, other, L.PlanRecord(other), t]) == sorted([t, other, other, t])
    assert {L.PlanRecord(other), r} - {t} == {other}


def test_wrong_family_access_raises():
    pipe, gather = L.PlanRecord(SAMPLES["conv_pipe"][0]), L.PlanRecord(SAMPLES["conv_gather"][0])
    for rec, name in ((gather, "lr"), (gather, "npi"), (pipe, "TILE"), (pipe, "ordered"), (pipe, "C_out"),
                      (L.PlanRecord(SAMPLES["head_fwd"][0]), "MT"), (L.PlanRecord(SAMPLES["wgrad_pipe"][0]), "flags"),
                      (L.PlanRecord(("fwd", 77) + (0,) * 11), "MT")):
        with pytest.raises(AttributeError):
            getattr(rec, name)


def test_ordered_truth_table():
    """`ordered` is the predicate the deterministic-mode tests spelled out by position:
    (r[1] == 8 and r[4] & 2) or (r[1] == 5 and r[3] == 1)."""
    def spelled_out(r):
        return bool((r[1] == 8 and r[4] & 2) or (r[1] == 5 and r[3] == 1))

    rows = [(("wgrad", 8, 2 | 32 << 8, 3, x4 | ws << 1, 8, 1, 5, 256, 65536, 9, 136, 2), bool(ws)) for x4 in (0, 1) for ws in (0, 1)]
    rows += [(("wgrad", 5, 2, part) + (0,) * 9, bool(part)) for part in (0, 1)]
    rows += [(SAMPLES["conv_wgrad"][0], False)]
    for t, want in rows:
        assert bool(L.PlanRecord(t).ordered) is want is spelled_out(t), t


def test_timer_family_is_a_function_of_the_kernel_ids():
    for kernels, fams, fam in (([3, 1], ("head", "pipe"), "pipe"), ([5], ("head",), "head"), ([8, 6], ("wgrad_pipe", "wgrad"), "wgrad_pipe"),
                               ([9], ("dconvt",), "dconvt"), ([], (), "other"), ([2, 7, 4], ("gather", "head", "head"), "gather"),
                               ([6, 3], ("wgrad", "head"), "wgrad"), ([9, 5], ("dconvt", "head"), "dconvt"), ([12], ("other",), "other")):
        assert L.timer_families(kernels) == (fams, fam), kernels


def test_logs_nest_and_restore(monkeypatch):
    """plan_log / geom_log without the library: the innermost receives, the outer is untouched, exit restores what it found."""
    monkeypatch.setattr(L, "lib", lambda: pytest.fail("the logs' bookkeeping loaded the library"))
    assert L.PLAN_LOG is None and C.GEOM_LOG is None
    outer = {("fwd", 1)}
    with L.plan_log(outer) as a:
        assert L.PLAN_LOG is outer is a.records and a.full_calls == []
        with L.plan_log() as b:
            assert L.PLAN_LOG is b.records and b.records == set() and b is not a
            L.PLAN_LOG.add(("dgrad", 2))
        assert L.PLAN_LOG is outer and outer == {("fwd", 1)} and b.records == {("dgrad", 2)}
        with pytest.raises(ZeroDivisionError):
            with L.plan_log():
                1 / 0
        assert L.PLAN_LOG is outer and L._PLAN_CAPTURE is a
    assert L.PLAN_LOG is None and L._PLAN_CAPTURE is None
    mine = []
    with C.geom_log(mine) as g:
        assert C.GEOM_LOG is mine is g
        with C.geom_log() as inner:
            assert C.GEOM_LOG is inner and inner == []
            C.GEOM_LOG.append("x")
        assert C.GEOM_LOG is mine and mine == [] and inner == ["x"]
        with pytest.raises(ZeroDivisionError):
            with C.geom_log():
                1 / 0
        assert C.GEOM_LOG is mine
    assert C.GEOM_LOG is None
