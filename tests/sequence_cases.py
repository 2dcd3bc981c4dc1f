"""Call order on one context ("Call order"): the subjects, the vocabulary of operations, the expected
results and the schedules of tests/test_gpu_call_sequences.py.  Pure numpy and the oracle: nothing here touches a GPU, and
tests/test_sequence_cases_cpu.py holds the census of what the schedules visit.

A SUBJECT is a small array with everything that is expected of it, computed once and never modified.  An OP is one public
method of dctz_amd.Context (or a knob, or a refused call) applied to a subject; a SCHEDULE is a list of (kind, subject,
arguments) and is plain data, so a failure can be replayed from its name and an index.

Expected results come from two sources, named per op kind in OPS:
  E1  the oracle or the numpy models of the feature tests (streams, every decode as a slice of the oracle's, mask words and
      filled arrays, correction lists, exact exception counts, deflate bytes against the twin);
  E2  the same op as the first work call of a fresh context, bit for bit (coarse decodes, summary records, predicted SSE and
      PSNR, compress_psnr's bound and measured value, psnr_terms, the coefficients of a QT call).  None of these reductions
      uses a floating-point atomic (the only atomics of the kernels are integer adds and maxima of bit patterns), their
      grids depend on the shape and the device alone, so two fresh contexts agree; the GPU module compares two once.
"""
import functools

import numpy as np

from oracle import oracle as O
from dctz_amd import hip as H
from tests import bin_edge_cases as BE
from tests import mask_cases as M
from tests import ndfix_cases as NF
from tests import ndmask_cases as NM

EB = 1e-3
TILE = 4096
SPEC_MIN = 1 << 18
HOLE = 1e36                             # the marker of a missing element; the rule is |x| >= LIMIT
LIMIT = 1e30
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)


def field(n, dtype, seed=11, gain=1.0):
    """test_gpu_decode_memo.field: a smooth field whose amplitude drifts from tile to tile, plus noise; two tiles of three carry
    a burst at the highest frequencies, tile 1 is bounded noise.  A short last block carries the burst too, so that it
    stores coefficients exactly like the tiles.  max|x| < 100 * gain."""
    t = np.arange(n) / 61.0
    rng = np.random.default_rng(seed + n)
    amp = 30.0 + 12.0 * np.sin(np.arange(n) / 9973.0)
    v = amp * (np.sin(t) + 0.3 * np.cos(5.3 * t)) + 0.4 * rng.standard_normal(n)
    burst = 30.0 * (1.0 - 2.0 * (np.arange(64) % 2))
    for tile in range(n // TILE):
        if tile % 3 != 2:
            v[tile * TILE + 5 * 64:tile * TILE + 6 * 64] += burst
    if n >= 2 * TILE:
        v[TILE:2 * TILE] = rng.uniform(-95.0, 95.0, TILE)
    if n % 64:
        v[n - n % 64:] += burst[:n % 64]
    return (gain * v).astype(dtype)


class Subject:
    """name; shape ((n,) for a flat array); dtype; mode; dims: the shape the flat box calls see it with; raw: the array with
    its holes (the input of the mask ops); x: the array the streams are of (raw with its holes filled; raw itself where there
    are none)."""

    def __init__(self, name, shape, dtype, mode, seed=11, gain=1.0, dims=None, holes=False):
        self.name, self.shape, self.dtype, self.mode = name, tuple(shape), np.dtype(dtype), mode
        self.flat = len(self.shape) == 1
        self.n = int(np.prod(self.shape))
        self.dims = tuple(dims) if dims else self.shape
        assert int(np.prod(self.dims)) == self.n
        v = field(self.n, self.dtype, seed, gain).reshape(self.shape)
        self.holes = holes
        if holes:
            rng = np.random.default_rng(seed)
            miss = rng.random(self.shape) < 0.07
            miss.reshape(-1)[64:128] = True               # a whole block / most of a tile row without a valid element
            miss.reshape(-1)[-1] = True
            v = np.where(miss, self.dtype.type(HOLE), v)
        self.raw = np.ascontiguousarray(v)
        miss = M.is_missing(self.raw, H.MISS_ABS_GE, 0.0, LIMIT)
        self.miss = miss
        self.x = np.ascontiguousarray((M.fill(self.raw, miss) if self.flat else NM.fill(self.raw, miss)) if holes else self.raw)
        self.n_lin = self.n if self.flat else 64 * NF.nblk(self.shape)      # positions the streams cover
        for a in (self.raw, self.x, self.miss):
            a.setflags(write=False)

    def __repr__(self):
        return f"<{self.name} {self.shape} {self.dtype} {'QT' if self.mode == O.QT else 'EC'}>"


BIG_N = (1 << 18) + 4096 + 1            # >= 4 * 1024 * 64 elements: the sampled guess of sf is taken in either element type
_SUBJECTS = [
    # flat: every (dtype, mode) at least twice, with different lengths of the short last block
    Subject("a27", (27,), F32, O.QT, dims=(3, 9)),                       # one short block only
    Subject("a64", (64,), F64, O.QT, dims=(8, 8)),
    Subject("a91", (91,), F32, O.EC, dims=(7, 13)),                      # fp32, short block of 27
    Subject("a2597", (40 * 64 + 37,), F32, O.EC, dims=(49, 53)),         # less than a tile; fp32, short block of 37
    Subject("a2597d", (40 * 64 + 37,), F64, O.EC, dims=(49, 53)),        # ... the same n in fp64
    Subject("h2597", (40 * 64 + 37,), F32, O.EC, seed=5, dims=(49, 53), holes=True),
    Subject("b12325", (3 * TILE + 37,), F64, O.QT, dims=(25, 493)),      # QT, large maxima
    Subject("b12325s", (3 * TILE + 37,), F64, O.QT, seed=3, gain=0.15, dims=(25, 493)),  # ... maxima a sixth of those
    Subject("q12325f", (3 * TILE + 37,), F32, O.QT, dims=(25, 493)),     # ... the same n in fp32
    Subject("c12288", (3 * TILE,), F64, O.EC, dims=(12, 32, 32)),        # eligible for the decode memo on the chain
    Subject("c12288b", (3 * TILE,), F64, O.EC, seed=4, dims=(12, 32, 32)),   # ... other content, for the same buffers
    Subject("big", (BIG_N,), F64, O.EC, dims=(3, BIG_N // 3)),           # sampled sf with set_speculation(True, 1 << 18)
    Subject("big32", (BIG_N,), F32, O.EC, dims=(3, BIG_N // 3)),
    # tiled
    Subject("t2r", (37, 70), F64, O.EC),                                 # 8 x 8, ragged
    Subject("t2a", (64, 128), F32, O.QT),                                # 8 x 8, aligned: two stream tiles
    Subject("t2h", (37, 70), F32, O.EC, seed=5, holes=True),
    Subject("t3r", (9, 14, 23), F32, O.EC),                              # 4 x 4 x 4, ragged: two stream tiles
    Subject("t3a", (16, 16, 32), F64, O.QT),                             # 4 x 4 x 4, aligned
]
SUBJECTS = {s.name: s for s in _SUBJECTS}
FLAT = [s.name for s in _SUBJECTS if s.flat]
TILED = [s.name for s in _SUBJECTS if not s.flat]
QT_PAIR = ("b12325", "b12325s")         # equal n and dtype, maxima more than 4 x apart
DTYPE_PAIR = ("b12325", "q12325f")      # equal n and mode, the other element type
REM_PAIR = ("a91", "a2597")             # equal dtype, short blocks of 27 and 37
MEMO_PAIR = ("c12288", "c12288b")       # equal n, dtype and mode: may share output buffers
ONE_WIDEST = "big"                      # most workgroups of a one-launch kernel
ONE_NARROW = "a91"


# ---- E1: expected results from the oracle and the numpy models ------------------------------------------------------------
def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def streams_at(name, eb, mode):
    """The oracle's streams of subject `name` at bound eb in `mode` (with the coefficients and the scaled copy)."""
    s = SUBJECTS[name]
    c = O.compress(s.x, eb, mode, O.FAST, want_coef=True) if s.flat else O.compress_nd(s.x, eb, mode, O.FAST)
    _ro(c.bin_index, c.dc, c.ac_exact, c.qtable, c.qtable_raw, c.coef, c.scaled)
    return c


def streams(name):
    return streams_at(name, EB, SUBJECTS[name].mode)


@functools.lru_cache(maxsize=None)
def decode(name):
    s = SUBJECTS[name]
    r = O.decompress(streams(name), O.FAST) if s.flat else O.decompress_nd(streams(name), s.shape, O.FAST)
    _ro(r)
    return r


def tile_counts(bin_index):
    """Per 4096 stream positions: flags 'stored exactly' (id 255 at j != 0), the short last block included."""
    n = bin_index.size
    f = (bin_index == 255) & (np.arange(n) % 64 != 0)
    m = -(-n // TILE)
    p = np.zeros(m * TILE, bool)
    p[:n] = f
    return p.reshape(m, TILE).sum(axis=1)


@functools.lru_cache(maxsize=None)
def index(name):
    """dctzhip_ac_index of the subject's streams: idx[i] = exact coefficients in front of position 4096 i; idx[-1] the total."""
    ix = np.concatenate([[0], np.cumsum(tile_counts(streams(name).bin_index))]).astype(np.int32)
    _ro(ix)
    return ix


@functools.lru_cache(maxsize=None)
def variant(name):
    """dctzhip_debug_counter 20 after a compress / compress_nd call of the subject."""
    s = SUBJECTS[name]
    return BE.variant(s.x, EB, s.dtype)


def box_of(name, lo, hi, nd):
    """The box of the decode: of the flat array seen as s.dims (nd False) or of the tiled array."""
    s = SUBJECTS[name]
    full = decode(name).reshape(s.shape if nd else s.dims)
    return np.ascontiguousarray(full[tuple(slice(l, h) for l, h in zip(lo, hi))])


@functools.lru_cache(maxsize=None)
def fix_bound(name, mult):
    """The absolute bound of the correction-list ops: mult times the largest error of the subject's decode."""
    s = SUBJECTS[name]
    return float(mult) * float(np.abs(s.x.astype(np.float64) - decode(name).astype(np.float64)).max())


@functools.lru_cache(maxsize=None)
def fix_list(name, mult):
    """(fix_start uint32[tiles + 1], fix_off uint16[count], fix_val T[count]) of the subject's decode against its array."""
    s = SUBJECTS[name]
    b = fix_bound(name, mult)
    if s.flat:
        q = np.flatnonzero(NF.listed(s.x, decode(name), b))
        m = -(-s.n // TILE)
        per = np.bincount(q // TILE, minlength=m).astype(np.uint64)
        start = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
        res = start, (q % TILE).astype(np.uint16), np.ascontiguousarray(s.x[q])
    else:
        res = NF.fix_list(s.x, decode(name), b)[1:]
    _ro(*res)
    return res


def fix_applied(name, mult):
    s = SUBJECTS[name]
    return NF.applied(s.x, decode(name), fix_bound(name, mult))


@functools.lru_cache(maxsize=None)
def mask(name):
    """(mask words uint64, count, the filled array) of the subject's raw array under |x| >= LIMIT."""
    s = SUBJECTS[name]
    w = M.mask_words(s.miss.reshape(-1))
    _ro(w)
    return w, int(s.miss.sum()), s.x


@functools.lru_cache(maxsize=None)
def dct_of(name, inverse):
    s = SUBJECTS[name]
    x = s.x.reshape(-1)
    y = np.empty_like(x)
    for b in range(0, s.n, 64):
        y[b:b + 64] = O.dct_inv(x[b:b + 64], O.FAST) if inverse else O.dct_fwd(x[b:b + 64], O.FAST)
    _ro(y)
    return y


@functools.lru_cache(maxsize=None)
def deflated(name):
    """Per section (bin_index, DC, AC_exact[:cnt]) of the subject's streams: (zlib stream, per-chunk sizes) of the twin."""
    from tests import containers
    L = containers.twin()
    c = streams(name)
    return [containers.twin_deflate(L, a.tobytes(), want_index=True) for a in (c.bin_index, c.dc, c.ac_exact)]


# ---- the vocabulary -----------------------------------------------------------------------------------------------------------
FAMILIES = ("compress", "decompress", "nd", "range", "box", "coarse", "summary", "fixup", "mask", "rd", "batch", "deflate")
E1, E2 = "E1", "E2"
RD_EBS = (1e-4, 1e-3, 1e-2)
PSNR_TARGET = 60.0


def _flat(s): return s.flat
def _tiled(s): return not s.flat
def _any(s): return True
def _small(s): return s.n <= 3 * TILE + 64


# kind -> (family, role, applies, source).  role: "compress" / "decode" for the census of knob states, None otherwise.
OPS = {
    "compress":          ("compress", "compress", _flat, E1),
    "compress_scaled":   ("compress", "compress", _flat, E1),      # scaled= out of place
    "compress_inplace":  ("compress", "compress", _flat, E1),      # scaled= the input itself, on a copy
    "compress_coef":     ("compress", "compress", _flat, E1),      # coef=: EC against the oracle, QT through E2
    "dct_blocks":        ("compress", None, _flat, E1),
    "decompress":        ("decompress", "decode", _flat, E1),
    "compress_nd":       ("nd", "compress", _tiled, E1),
    "decompress_nd":     ("nd", "decode", _tiled, E1),
    "range":             ("range", "decode", _flat, E1),           # ac_index + decompress_range
    "box":               ("box", "decode", _flat, E1),
    "boxes":             ("box", "decode", _flat, E1),
    "box_nd":            ("box", "decode", _tiled, E1),
    "boxes_nd":          ("box", "decode", _tiled, E1),
    "coarse":            ("coarse", "decode", _flat, E2),
    "coarse_nd":         ("coarse", "decode", _tiled, E2),
    "coarse_box_nd":     ("coarse", "decode", _tiled, E2),         # (E2 of coarse_nd at the same factor, sliced on the host)
    "coarse_boxes_nd":   ("coarse", "decode", _tiled, E2),
    "summary":           ("summary", "decode", _flat, E2),
    "summary_ref":       ("summary", "decode", _flat, E2),
    "summary_nd":        ("summary", "decode", _tiled, E2),
    "summary_nd_ref":    ("summary", "decode", _tiled, E2),
    "fixup_count":       ("fixup", "decode", _flat, E1),
    "fixup_list":        ("fixup", "decode", _flat, E1),
    "fixup_apply":       ("fixup", None, _flat, E1),
    "fixup_count_nd":    ("fixup", "decode", _tiled, E1),
    "fixup_list_nd":     ("fixup", "decode", _tiled, E1),
    "fixup_apply_nd":    ("fixup", None, _tiled, E1),
    "mask_build":        ("mask", None, _flat, E1),
    "mask_build_nd":     ("mask", None, _tiled, E1),
    "compress_masked":   ("mask", "compress", _flat, E1),          # without filled=: the library's own copy
    "compress_masked_nd": ("mask", "compress", _tiled, E1),
    "mask_apply":        ("mask", None, _any, E1),
    "rd_probe":          ("rd", None, _flat, E2),                  # (the exception counts: E1)
    "rd_probe_nd":       ("rd", None, _tiled, E2),
    "compress_psnr":     ("rd", "compress", _flat, E2),            # (the streams at the chosen bound: E1)
    "compress_psnr_nd":  ("rd", "compress", _tiled, E2),
    "psnr_terms":        ("rd", None, _any, E2),
    "compress_batch":    ("batch", "compress", _flat, E1),
    "decompress_batch":  ("batch", "decode", _flat, E1),
    "deflate":           ("deflate", None, _small, E1),
    "inflate":           ("deflate", None, _small, E1),
}
# ops that are not calls of work but change what the next calls do: kind -> (knob, value)
STATE_OPS = {
    "one_on": ("one", 1), "one_off": ("one", 0),
    "spec_on": ("spec", 1), "spec_off": ("spec", 0),               # set_speculation(on, SPEC_MIN)
    "specmem_on": ("specmem", 1), "specmem_off": ("specmem", 0),
    "memo_on": ("memo", 1), "memo_off": ("memo", 0),
    "split_on": ("split", 1), "split_off": ("split", 0),
    "set_stream": (None, None),                                    # the same stream again
    "cooldown": (None, None),                                      # knob(2, k): k calls on the chain pending
    "withheld": (None, None),                                      # knob(0, 1) for one compress or decompress call, then back
}
KNOB_DEFAULTS = {"one": 1, "spec": 1, "specmem": 1, "memo": 1, "split": 0}
# refused calls, each asserting its error code: only what the argument-check tests and tests/golden/refusal_texts.json send
REFUSALS = {
    "ref_null": H.E_ARG,            # decompress_range, output NULL
    "ref_misaligned": H.E_ARG,      # decompress_range, output 4 bytes off a 16-byte boundary
    "ref_lohi": H.E_ARG,            # decompress_range, lo == hi
    "ref_space": H.E_SPACE,         # fixup_build with room for one entry less than the list has
    "ref_sections": H.E_ARG,        # deflate of 9 sections
}
KINDS = tuple(OPS) + tuple(STATE_OPS) + tuple(REFUSALS)
KINDS_OF = {f: [k for k, v in OPS.items() if v[0] == f] for f in FAMILIES}


def family(kind):
    return OPS[kind][0] if kind in OPS else None


def applies(kind, name):
    s = SUBJECTS[name]
    if kind in OPS:
        return bool(OPS[kind][2](s))
    if kind in ("ref_null", "ref_misaligned", "ref_lohi", "ref_space", "withheld"):
        return s.flat and (kind != "withheld" or s.n >= 64)
    return False


def coarse_shape(shape, factor):
    return tuple(-(-int(v) // factor) for v in shape)


def _rand_box(rng, dims):
    lo, hi = [], []
    for d in dims:
        a = int(rng.integers(0, d))
        b = int(rng.integers(a + 1, d + 1))
        lo.append(a)
        hi.append(b)
    return lo, hi


def batch_members(rng, mode):
    """Three flat subjects of one mode (a batch call has one), both element types among them, no buffer twice.  (The directed
    schedules also hold batches of one and two arrays.)"""
    pool = [n for n in FLAT if SUBJECTS[n].mode == mode and n != "c12288b"]
    while True:
        pick = [pool[i] for i in rng.choice(len(pool), 3, replace=False)]
        if len({SUBJECTS[n].dtype for n in pick}) == 2:
            return pick


def make_args(kind, name, rng):
    """The arguments of one op, drawn from rng: plain data (ints, floats, lists, strings)."""
    s = SUBJECTS[name] if name else None
    if kind == "range":
        lo = int(rng.integers(0, s.n))
        return {"lo": lo, "hi": int(rng.integers(lo + 1, s.n + 1))}
    if kind in ("box", "box_nd"):
        lo, hi = _rand_box(rng, s.dims if kind == "box" else s.shape)
        return {"lo": lo, "hi": hi}
    if kind in ("boxes", "boxes_nd"):
        return {"boxes": [list(_rand_box(rng, s.dims if kind == "boxes" else s.shape)) for _ in range(3)]}
    if kind == "coarse":
        return {"factor": int(rng.choice([2, 64]))}
    if kind == "coarse_nd":
        return {"factor": int(rng.choice([2, 8 if len(s.shape) == 2 else 4]))}
    if kind in ("coarse_box_nd", "coarse_boxes_nd"):                   # boxes in coarse coordinates; the tile edge is the DC-only factor
        f = int(rng.choice([2, 4, 8] if len(s.shape) == 2 else [2, 4]))
        ext = coarse_shape(s.shape, f)
        if kind == "coarse_box_nd":
            lo, hi = _rand_box(rng, ext)
            return {"factor": f, "lo": lo, "hi": hi}
        return {"factor": f, "boxes": [list(_rand_box(rng, ext)) for _ in range(3)]}
    if kind.startswith("fixup") or kind == "ref_space":
        return {"mult": float(rng.choice([0.25, 0.5]))}
    if kind == "mask_apply":
        return {"fill": float(rng.choice([-1.0, 9999.0]))}
    if kind in ("compress_batch", "decompress_batch"):
        return {"members": batch_members(rng, s.mode)}
    if kind == "dct_blocks":
        return {"inverse": bool(rng.integers(0, 2))}
    if kind == "cooldown":
        return {"calls": int(rng.integers(0, 4))}
    if kind == "withheld":
        return {"call": str(rng.choice(["compress", "decompress"]))}
    return {}


def e2_key(kind, name, args):
    """What an E2 result depends on: the op, the subject and the arguments that change the computation."""
    return (kind, name) + tuple(sorted((k, v) for k, v in args.items() if k in ("factor",)))


# ---- schedules --------------------------------------------------------------------------------------------------------------
WALK_SEEDS = (9, 10, 11, 12, 13, 14, 15, 16)           # (the first run of eight consecutive seeds that meets the census)
WALK_LEN = 120


def op(kind, name=None, **args):
    return (kind, name, dict(args))


def walk(seed, length=WALK_LEN):
    """A random walk over the vocabulary: about one op in eight changes a knob, one in sixteen is a refused call, the others
    are work ops whose family is drawn first (so that the families, not the kinds, are equally likely), then the kind, then a
    subject the kind applies to.  Nothing is emitted that the runner would have to leave out."""
    rng = np.random.default_rng(seed)
    sched = []
    while len(sched) < length:
        r = rng.random()
        if r < 0.125:
            kind = str(rng.choice(list(STATE_OPS)))
            name = str(rng.choice([n for n in FLAT if applies("withheld", n) and SUBJECTS[n].n <= 3 * TILE + 64])) if kind == "withheld" else None
        elif r < 0.1875:
            kind = str(rng.choice(list(REFUSALS)))
            name = str(rng.choice([n for n in FLAT if applies(kind, n)])) if kind != "ref_sections" else None
        else:
            fam = FAMILIES[int(rng.integers(0, len(FAMILIES)))]
            kind = str(rng.choice(KINDS_OF[fam]))
            name = str(rng.choice([n for n in SUBJECTS if applies(kind, n)]))
        sched.append((kind, name, make_args(kind, name, rng)))
    return sched


def _every_family(rng, flat_name, nd_name):
    """One op of every family (the tiled ones on nd_name)."""
    ops = []
    for fam in FAMILIES:
        kinds = KINDS_OF[fam]
        kind = kinds[int(rng.integers(0, len(kinds)))]
        name = flat_name if applies(kind, flat_name) else nd_name
        if not applies(kind, name):
            name = next(n for n in SUBJECTS if applies(kind, n))
        ops.append((kind, name, make_args(kind, name, rng)))
    return ops


def _decode_families(name, rng):
    """Every decode family of a flat subject."""
    return [(k, name, make_args(k, name, rng)) for k in
            ("decompress", "range", "box", "boxes", "coarse", "summary", "summary_ref", "fixup_count", "fixup_list", "deflate")]


def _ladder(order):
    """For every family with a capacity of its own, the subjects in `order` (flat, tiled)."""
    rng = np.random.default_rng(7)
    ops = []
    for kind in ("compress", "decompress", "range", "boxes", "coarse", "summary", "summary_ref", "fixup_list", "mask_build", "compress_masked",
                 "rd_probe", "compress_psnr", "deflate", "dct_blocks"):
        for name in order[0]:
            if applies(kind, name):
                ops.append((kind, name, make_args(kind, name, rng)))
    for kind in ("compress_nd", "decompress_nd", "boxes_nd", "coarse_nd", "summary_nd_ref", "fixup_list_nd", "mask_build_nd", "compress_masked_nd",
                 "rd_probe_nd", "compress_psnr_nd"):
        for name in order[1]:
            ops.append((kind, name, make_args(kind, name, rng)))
    large, small = ["big", "big32", "a2597d"], ["a91", "a2597d", "a2597"]            # the batch blobs and control blocks
    for members in ((large, small, large) if order[0][0] == "big" else (small, large, small)):
        ops += [("compress_batch", members[0], {"members": members}), ("decompress_batch", members[0], {"members": members})]
    return ops


def _alternate(pair, times, chain):
    a, b = pair
    ops = [op("one_off" if chain else "one_on")]
    for _ in range(times):
        for name in (a, b):
            ops += [op("compress", name), op("decompress", name)]
    return ops


def directed():
    """name -> (schedule, contexts): the directed schedules; contexts > 1: the ops carry the context they run on ("ctx")."""
    rng = np.random.default_rng(2024)
    d = {}
    # (a) capacity ladder: largest, smallest, largest -- and smallest first on a context of its own
    d["a_ladder_large_first"] = _ladder((["big", "a27", "big32", "c12288", "a91", "b12325"], ["t2a", "t2r", "t2a", "t3a", "t3r", "t3a"]))
    d["a_ladder_small_first"] = _ladder((["a27", "big", "a91", "big32", "a64", "b12325"], ["t2r", "t2a", "t2r", "t3r", "t3a", "t3r"]))
    # (b) the same n, the element type flips, in QT: on the one-launch path and on the chain (qt_item's bytes, rtab_dtype)
    d["b_dtype_flip_qt"] = _alternate(DTYPE_PAIR, 3, chain=False) + _alternate(DTYPE_PAIR, 3, chain=True) + [
        op("compress_batch", "b12325", members=["b12325", "q12325f", "a27"]), op("decompress_batch", "b12325", members=["b12325", "q12325f", "a27"]),
        op("compress", "q12325f"), op("decompress", "b12325"), op("range", "q12325f", lo=12200, hi=12325), op("range", "b12325", lo=12200, hi=12325)]
    # (c) the length of the short block changes, the element type does not: single calls and batches (rtab_l, rtab_cache)
    c = []
    for chain in (False, True):
        c.append(op("one_off" if chain else "one_on"))
        for _ in range(2):
            for name in REM_PAIR:
                c += [op("compress", name), op("decompress", name), op("range", name, lo=SUBJECTS[name].n - 30, hi=SUBJECTS[name].n),
                      op("coarse", name, factor=2)]
            c += [op("compress_batch", "a91", members=["a91", "a2597d", "a2597"]), op("decompress_batch", "a91", members=["a91", "a2597d", "a2597"]),
                  op("decompress", "a2597"), op("compress_batch", "a2597", members=["a2597", "a2597d", "h2597"]), op("decompress", "a91")]
    d["c_remainder_lengths"] = c
    # (d) QT: the large and the small maxima alternate six times -- one launch, chain, batches (one_cslot, one_qt, one_bqt, qtab)
    dq = _alternate(QT_PAIR, 6, chain=False) + _alternate(QT_PAIR, 6, chain=True)
    for chain in (False, True):
        dq.append(op("one_off" if chain else "one_on"))
        for i in range(6):                                # (a batch's tables are per item: the pair alternates at item 0)
            a, b = QT_PAIR if i % 2 == 0 else QT_PAIR[::-1]
            m = [a, "q12325f", "a64"] if i % 2 == 0 else [a, "a27", "a64"]
            dq += [op("compress_batch", m[0], members=m), op("decompress_batch", m[0], members=m), op("compress", b), op("decompress", b)]
        # ... and a batch of fewer arrays in between: the entries of a half that the shorter call's hand-off does not reach
        # (one_bdirty) hold the large maxima when the small ones come to them
        for m in ([QT_PAIR[1], QT_PAIR[0], "a64"], ["a64"], [QT_PAIR[0], QT_PAIR[1], "a64"], ["q12325f", "a27"], [QT_PAIR[1], QT_PAIR[0], "a64"]):
            dq += [op("compress_batch", m[0], members=m), op("decompress_batch", m[0], members=m)]
    d["d_qt_maxima"] = dq
    # (e) after each refusal, after the withheld granule and during its cooldown: one op of every family
    e = []
    for kind in REFUSALS:
        name = None if kind == "ref_sections" else "b12325" if kind != "ref_space" else "a2597d"
        e.append((kind, name, make_args(kind, name, rng)))
        e += _every_family(rng, "a2597d" if kind != "ref_space" else "b12325", "t2r")
    e += [op("one_on"), op("compress", "c12288"), op("withheld", "c12288", call="compress")] + _every_family(rng, "c12288", "t3r")
    e += [op("cooldown", calls=0), op("compress", "b12325"), op("withheld", "b12325", call="decompress")] + _every_family(rng, "b12325", "t3a")
    d["e_after_refusals"] = e
    # (f) every decode family on A after a compress of B into other buffers, then after a compress of B into the SAME buffers
    # (the memo's pointers match what the decode passes): B's decode
    a, b = MEMO_PAIR
    f = []
    for chain in (True, False):
        f.append(op("one_off" if chain else "one_on"))
        f += [op("compress", a, slot="shared")] + [(k, n_, dict(g, slot="shared")) for k, n_, g in _decode_families(a, rng)]
        f += [op("compress", b)] + [(k, n_, dict(g, slot="shared")) for k, n_, g in _decode_families(a, rng)]
        f += [op("compress", a, slot="shared"), op("compress", b, slot="shared")] + [(k, n_, dict(g, slot="shared")) for k, n_, g in _decode_families(b, rng)]
        f += [op("compress", a, slot="shared"), op("compress_batch", b, members=[b, "a2597", "a91"], slots=["shared", "a2597", "a91"]),
              op("decompress", b, slot="shared")]
    d["f_same_buffers"] = f
    # (g) two contexts on two streams of one device, the ops alternating between them
    g = []
    w0, w1 = walk(901, 40), walk(902, 40)
    for (k0, n0, a0), (k1, n1, a1) in zip(w0, w1):
        g += [(k0, n0, dict(a0, ctx=0)), (k1, n1, dict(a1, ctx=1))]
    d["g_two_contexts"] = g
    return d


def all_schedules():
    s = {f"walk_{seed}": walk(seed) for seed in WALK_SEEDS}
    s.update(directed())
    return s


def epoch_wrap():
    """The wrap of the one-launch tag (dctzhip_debug_knob 4; "epoch" is this schedule's own op, not one of the vocabulary).
    The widest one-launch subject runs at tag 1 on the fresh context and leaves a granule with that tag at every workgroup
    index.  The tag is set to 2^32 - 3; four narrow calls take 2^32 - 2, 2^32 - 1, 1 (the wrap) and 2 and rewrite the first
    two indices only.  Then every form of a wide call is made to take tag 1 itself (the tag set to 2^32 - 1 in front of
    it), each behind a wide call of OTHER content at tag 1: without the clearing of the board on the wrap, its sweeps would
    take that call's granules -- exception counts that place AC_exact -- for this launch's."""
    last = (1 << 32) - 1
    wide = [ONE_WIDEST, "big32", "a2597d"]
    return ([op("compress", ONE_WIDEST), op("epoch", value=(1 << 32) - 3)]
            + [op("compress", ONE_NARROW), op("decompress", ONE_NARROW), op("compress", ONE_NARROW), op("decompress", ONE_NARROW)]
            + [op("epoch", value=last), op("compress", "big32"), op("epoch", value=last), op("decompress", ONE_WIDEST),
               op("epoch", value=last), op("compress", ONE_WIDEST), op("epoch", value=last), op("decompress", "big32"),
               op("epoch", value=last), op("compress_batch", ONE_WIDEST, members=wide), op("epoch", value=last), op("compress", "big32"),
               op("epoch", value=last), op("decompress_batch", ONE_WIDEST, members=wide)])


# ---- the census: what a set of schedules visits (tests/test_sequence_cases_cpu.py asserts it for the walks) -----------------
def targets(kind, name, args):
    """The subjects an op works on."""
    if kind in ("compress_batch", "decompress_batch"):
        return list(args["members"])
    return [name] if name else []


def census(schedules):
    """kinds: occurrences per kind; pairs: occurrences per (family of the previous work op, family of this one), within a
    schedule; compressed / decoded: subjects that were the target of a compress / of a decode; knobs: per (knob, value),
    [compress ops, decode ops] that ran while it held; inapplicable: emitted ops the runner could not run."""
    kinds = {k: 0 for k in KINDS}
    pairs = {(a, b): 0 for a in FAMILIES for b in FAMILIES}
    compressed, decoded = set(), set()
    knobs = {(k, v): [0, 0] for k in KNOB_DEFAULTS for v in (0, 1)}
    inapplicable = 0
    for sched in schedules:
        state = dict(KNOB_DEFAULTS)
        prev = None
        for kind, name, args in sched:
            kinds[kind] += 1
            if kind in STATE_OPS:
                knob, value = STATE_OPS[kind]
                if knob:
                    state[knob] = value
            if kind in OPS:
                fam, role = OPS[kind][0], OPS[kind][1]
                for t in targets(kind, name, args):
                    if not applies(kind, t):
                        inapplicable += 1
                if prev is not None:
                    pairs[(prev, fam)] += 1
                prev = fam
                if role:
                    (compressed if role == "compress" else decoded).update(targets(kind, name, args))
                    for k, v in state.items():
                        knobs[(k, v)][0 if role == "compress" else 1] += 1
            elif name is not None and not applies(kind, name):
                inapplicable += 1
    return {"kinds": kinds, "pairs": pairs, "compressed": compressed, "decoded": decoded, "knobs": knobs, "inapplicable": inapplicable}


# ---- stream order (tests/test_gpu_stream_order.py; DESIGN.md section 4, "Stream order") -------------------------------------
STREAM_REPLAY = ("walk_9", "walk_10", "d_qt_maxima", "f_same_buffers", "e_after_refusals")
STREAM_WALK = (2, 60)                   # (the first seed whose 60 ops bring set_speculation(off) a compress and a decode, and
                                        # every kind its second occurrence: the subset then meets its census)
HOP_WALK = "walk_11"
# spec memory across a change of decade: `big` two decades up lives in the same device buffer as `big` (not in SUBJECTS: the
# walks draw their subjects from there, and stay what they are)
BIG_UP = Subject("big_up", (BIG_N,), F64, O.EC, gain=100.0, dims=(3, BIG_N // 3))


def stream_schedules():
    """name -> schedule: what is replayed with producers pending on the stream and the buffers recycled behind every call."""
    a = all_schedules()
    d = {n: a[n] for n in STREAM_REPLAY}
    d["walk_%d_%d" % STREAM_WALK] = walk(*STREAM_WALK)
    return d


def hop_stream(i):
    """h_stream_hops: the stream op i of HOP_WALK runs on -- 0 / 1 two streams of the caller's, 2 the legacy default stream."""
    return 2 if i % 3 == 2 else (i - i // 3) % 2
