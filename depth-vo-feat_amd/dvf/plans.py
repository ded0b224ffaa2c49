"""The convolution plan record of dvf_conv2d_last_plans, named: the host mirror of the table above that entry in
include/dvf_hip.h (tests/test_plan_record.py holds the two together).  No GPU and no library here; dvf.lib re-exports it."""

PLAN_INTS, PLAN_MAX = 12, 8
K_PIPE, K_GATHER, K_HEAD_FWD, K_HEAD_DGRAD, K_HEAD_WGRAD, K_WGRAD, K_HEAD_SEG_DGRAD, K_WGRAD_PIPE, K_DCONVT_FWD = range(1, 10)
KERNELS = {K_PIPE: "conv_pipe", K_GATHER: "conv_gather", K_HEAD_FWD: "head_fwd", K_HEAD_DGRAD: "head_dgrad",
           K_HEAD_WGRAD: "head_wgrad", K_WGRAD: "conv_wgrad", K_HEAD_SEG_DGRAD: "head_seg_dgrad", K_WGRAD_PIPE: "wgrad_pipe",
           K_DCONVT_FWD: "dconvt_fwd"}

PLAN_MODE_MASK, PLAN_NCLS_SHIFT, PLAN_NCLS_MASK = 15, 4, 15
PLAN_X4_SHIFT, PLAN_BLOCKED_SHIFT, PLAN_LR_SHIFT, PLAN_NPI_SHIFT = 8, 9, 10, 11
PLAN_WG_MT_MASK, PLAN_WG_TILE_SHIFT, PLAN_WG_X4_SHIFT, PLAN_WG_ORDERED_SHIFT = 255, 8, 0, 1
OUT_MODES = ("fused", "atomic", "ws")

_MFMA = ("MT", "NT", "WM", "CK", "TBU", "KS", "BN", "NST", "threads", "lds", "flags")
PLAN_FIELDS = {      # kernel -> names of the ints after it, in order
    K_PIPE: _MFMA,
    K_GATHER: _MFMA,
    K_HEAD_FWD: ("C_out", "nseg"),
    K_HEAD_DGRAD: ("C_out",),
    K_HEAD_WGRAD: ("C_out", "ordered"),
    K_WGRAD: ("MT", "NTW", "prefetch", "CK", "BH", "PSPLIT", "vec_p", "stride", "threads", "lds", "taps"),
    K_HEAD_SEG_DGRAD: ("segc",),
    K_WGRAD_PIPE: ("tile", "NTW", "lanes", "CK", "stride", "pieces", "blocks", "lds", "taps", "row_stride", "nseg"),
    K_DCONVT_FWD: ("C_out", "KH"),
}
_MODE = ("flags", 0, PLAN_MODE_MASK, OUT_MODES.__getitem__)
_NCLS = ("flags", PLAN_NCLS_SHIFT, PLAN_NCLS_MASK, int)
PLAN_PACKED = {      # kernel -> sub-field -> (word, shift, mask or None for "the rest", conversion)
    K_PIPE: {"out_mode": _MODE, "ncls": _NCLS, "x4": ("flags", PLAN_X4_SHIFT, 1, bool),
             "blocked": ("flags", PLAN_BLOCKED_SHIFT, 1, bool), "lr": ("flags", PLAN_LR_SHIFT, 1, bool),
             "npi": ("flags", PLAN_NPI_SHIFT, None, int)},
    K_GATHER: {"out_mode": _MODE, "ncls": _NCLS},
    K_WGRAD: {"ordered": ("MT", 0, 0, bool)},        # never: this weight-gradient kernel has float atomics only (mask 0)
    K_WGRAD_PIPE: {"MT": ("tile", 0, PLAN_WG_MT_MASK, int), "TILE": ("tile", PLAN_WG_TILE_SHIFT, None, int),
                   "x4": ("lanes", PLAN_WG_X4_SHIFT, 1, bool), "ordered": ("lanes", PLAN_WG_ORDERED_SHIFT, 1, bool)},
}


class PlanRecord(tuple):
    """(op, kernel, 11 ints): one launch of a convolution call.  It compares, hashes and sorts as that plain tuple; the ints
    are read by the names of the record's own kernel family (PLAN_FIELDS, PLAN_PACKED), any other name is an AttributeError."""
    __slots__ = ()
    op = property(lambda self: self[0])
    kernel = property(lambda self: self[1])
    kernel_name = property(lambda self: KERNELS[self[1]])

    def __getattr__(self, name):
        fields = PLAN_FIELDS.get(self[1], ())
        if name in fields:
            return self[2 + fields.index(name)]
        sub = PLAN_PACKED.get(self[1], {}).get(name)
        if sub is None:
            raise AttributeError("a %s plan record has no field %r" % (KERNELS.get(self[1], self[1]), name))
        word, shift, mask, conv = sub
        v = self[2 + fields.index(word)] >> shift
        return conv(v if mask is None else v & mask)


def records_of(buf, n, op=None):
    """The records in the first n ints that dvf_conv2d_last_plans wrote to buf."""
    return [PlanRecord((op,) + tuple(buf[i:i + PLAN_INTS])) for i in range(0, n, PLAN_INTS)]


TIMER_FAMILY = {K_PIPE: "pipe", K_GATHER: "gather", K_HEAD_FWD: "head", K_HEAD_DGRAD: "head", K_HEAD_WGRAD: "head",
                K_WGRAD: "wgrad", K_HEAD_SEG_DGRAD: "head", K_WGRAD_PIPE: "wgrad_pipe", K_DCONVT_FWD: "dconvt"}


def timer_families(kernels):
    """KernelTimer's name of every launch of a call, and of the call: the kernel family with the most work."""
    fams = tuple(TIMER_FAMILY.get(k, "other") for k in kernels)
    return fams, next((f for f in ("pipe", "wgrad_pipe", "gather", "wgrad", "dconvt", "head") if f in fams), "other")
