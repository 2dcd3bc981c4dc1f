"""Arrays past the resident grid, past 2 GiB and past 4 GiB, predicted from a model of one period (tests/test_gpu_size_edges_*.py,
tests/test_gpu_coarse_decode.py, tests/test_size_cases_cpu.py).

No reference runs on 4 GiB of doubles in test time, but blocks are independent once sf is fixed.  A big array B is a pattern P
repeated `reps` times along its first axis, followed by a tail that is a PREFIX of P; the model S = [P | tail] is small enough
for the independent references (the oracle, the numpy restatements of the other *_cases.py files).  max |B| = max |S| (the tail
adds no value P has not), so sf is S's, and every per-block and per-tile output of B is, bit for bit, the corresponding output of
S: S's first period `reps` times, then S's tail.  Running counts (the exception index, fix_start) advance by the period's count.

Everything here takes numpy arrays or torch tensors alike: the CPU file feeds the references' outputs on a miniature B, the GPU
files the library's outputs on the real one (compared on the device; only tile tables and small pieces come to the host).

Flat arrays: a period is a whole number of 4096-element stream tiles.  Tiled arrays (8 x 8 / 4 x 4 x 4): a period is a number of
rows / planes whose blocks fill whole stream tiles; the streams are block-linear (row-major over the tile grid), so a period of
the array IS a period of the streams, and the ragged rows at the far end are the model's tail.
"""
import numpy as np

TILE, BLK = 4096, 64
EDGE = {2: 8, 3: 4}
EB = 1e-3
FOUR_GIB = 1 << 32
ND_WINDOW = 0xFFFFF000                # the largest tiled array (bytes) the kernels address in place (dctz_shim.hip: nd_direct)


class Workload:
    """shape: the big array's; period: elements (flat) or rows / planes (tiled) of one repeat along axis 0."""

    def __init__(self, name, shape, period, tiled, views=()):
        self.name, self.shape, self.period, self.tiled = name, tuple(int(v) for v in shape), int(period), bool(tiled)
        self.views = tuple(views)                                   # flat: the shapes the box calls see it with
        self.reps, self.tail = divmod(self.shape[0], self.period)
        self.rest = self.shape[1:]
        self.row = int(np.prod(self.rest, dtype=np.int64))          # elements per unit of axis 0
        self.n = self.shape[0] * self.row
        self.model_shape = (self.period + self.tail,) + self.rest
        self.elem_per = self.period * self.row                      # elements of a period, in C order
        if tiled:
            e = EDGE[len(self.shape)]
            assert self.period % e == 0
            nb_rest = int(np.prod([-(-d // e) for d in self.rest], dtype=np.int64))
            self.stream_per = self.period // e * nb_rest * BLK
            self.stream_n = -(-self.shape[0] // e) * nb_rest * BLK
        else:
            assert not self.rest
            self.stream_per, self.stream_n = self.period, self.n
        self.stream_tail = self.stream_n - self.reps * self.stream_per
        self.model_stream_n = self.stream_per + self.stream_tail
        self.tiles_per = self.stream_per // TILE
        self.tiles = -(-self.stream_n // TILE)
        self.bytes = 8 * self.n                                     # fp64 throughout

    def check(self, past=FOUR_GIB, ragged=True):
        """The conditions every workload meets: whole stream tiles per period (per-tile outputs are periodic too); mask words
        do not straddle periods; the tail is a prefix of the pattern; 2^32 bytes (`past`) is not a whole number of periods, so
        an offset that wraps or sign-extends lands on other data; the far end is ragged wherever the shape allows."""
        assert self.reps >= 2 and self.stream_per % TILE == 0 and self.tiles_per >= 1, self.name
        assert self.elem_per % BLK == 0 and 0 <= self.tail < self.period, self.name
        assert past % (8 * self.elem_per) != 0, self.name
        if ragged and not self.tiled:
            assert self.n % BLK != 0 and self.tail > BLK, self.name
        if ragged and self.tiled:
            e = EDGE[len(self.shape)]
            assert all(d % e for d in self.shape), self.name
        for v in self.views:
            assert int(np.prod(v, dtype=np.int64)) == self.n, (self.name, v)
        return self

    def prefix(self, reps):
        """The same construction with fewer repeats: the array-side prefix of this one."""
        return Workload(f"{self.name}[:{reps}]", (reps * self.period + self.tail,) + self.rest, self.period, self.tiled)


# ---- the workloads (fp64) ----
F = Workload("F", (537929784,), 4096 * 257, False, views=((537929784,), (261639, 2056), (261639, 257, 8), (87213, 3, 257, 8)))
A2 = Workload("A2", (699072, 576), 64, True)
A3 = Workload("A3", (27968, 100, 144), 64, True)
G2 = Workload("G2", (65541, 8203), 256, True)
G3 = Workload("G3", (36739, 101, 145), 128, True)
G3A = Workload("G3a", (37376, 100, 144), 64, True)
C = Workload("C", (8195 * 4096 + 5 * 64 + 37,), 4096 * 257, False)
G2_COARSE = G2.prefix(33)              # (8453, 8203): 16 929 tiles + the ragged rows
G3_COARSE = G3.prefix(18)              # (2307, 101, 145)
# 256 CUs x 32 waves: what the card holds of single-wave workgroups at once, whatever a kernel's occupancy
RESIDENT_WAVES = 256 * 32
DC_GRID_BLOCKS = 4096 * 256            # blocks one trip of k_decompress_coarse_dc covers (dctz_kernels_coarse.hip)

# the same constructions with 3 repeats and periods of a few tiles (the CPU file): flat with a short block, 8 x 8 and 4 x 4 x 4
# tiles ragged on every axis
MINI_F = Workload("f", (3 * 3 * 4096 + 4096 + 2 * 64 + 56,), 3 * 4096, False)
MINI_G2 = Workload("g2", (3 * 512 + 5, 131), 512, True)
MINI_G3 = Workload("g3", (3 * 64 + 3, 9, 13), 64, True)


def check_workloads():
    """The arithmetic of the table of workloads."""
    F.check()
    assert F.n % 64 == 56 and F.bytes == 4303438272 and (F.reps, F.tail, F.tiles_per) == (511, 14392, 257)
    assert 2056 % 64 and 512 * 2056 == F.period                                # blocks straddle rows; one period is 512 rows
    assert (F.reps - 1) * F.period * 8 < FOUR_GIB < F.reps * F.period * 8      # the 4 GiB line lies inside the last period
    for w, nbytes, reps, tail, tiles_per in ((A2, 3221323776, 10923, 0, 9), (A3, 3221913600, 437, 0, 225)):
        w.check(ragged=False)
        w.check(past=1 << 31, ragged=False)
        assert (w.bytes, w.reps, w.tail, w.tiles_per) == (nbytes, reps, tail, tiles_per), w.name
        assert (1 << 31) < w.bytes <= ND_WINDOW, w.name                        # inside the in-place window, past 2 GiB
    G2.check()
    assert (G2.bytes, G2.reps, G2.tail, G2.tiles_per) == (4301062584, 256, 5, 513) and G2.tiles == 131345
    G3.check()
    assert (G3.bytes, G3.reps, G3.tail, G3.tiles_per) == (4304341240, 287, 3, 481)
    G3A.check(ragged=False)
    assert (G3A.bytes, G3A.reps, G3A.tail, G3A.tiles_per) == (4305715200, 584, 0, 225) and G3A.bytes > ND_WINDOW
    for w in (G2, G3, G3A):
        assert w.bytes > FOUR_GIB, w.name
    C.check(past=1 << 31)
    # (C's 524 485 blocks are ONE trip of the DC kernel; the tiled prefix of G2 below is the workload that makes it stride)
    assert C.tiles > RESIDENT_WAVES and (C.reps, C.tiles_per) == (31, 257)
    G2_COARSE.check(past=1 << 31)
    G3_COARSE.check(past=1 << 31)
    assert G2_COARSE.shape == (8453, 8203) and G2_COARSE.reps * G2_COARSE.tiles_per == 16929
    assert G3_COARSE.shape == (2307, 101, 145) and G3_COARSE.reps == 18
    assert G2_COARSE.tiles > RESIDENT_WAVES and G3_COARSE.tiles > RESIDENT_WAVES
    assert G2_COARSE.stream_n // 64 > DC_GRID_BLOCKS                           # the DC kernel strides
    for w in (MINI_F, MINI_G2, MINI_G3):
        w.check(past=1 << 20)
        assert w.reps == 3


# ---- numpy arrays and torch tensors alike ----
def _torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def bits(a):
    """Floats as integers of their size (a NaN equals itself, -0.0 differs from +0.0); integers as they are."""
    if _torch(a):
        import torch
        return a.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(a.dtype, a.dtype))
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    a, b = bits(a), bits(b)
    if _torch(a):
        import torch
        return tuple(a.shape) == tuple(b.shape) and bool(torch.equal(a, b))
    return a.shape == b.shape and bool(np.array_equal(a, b))


def expand(s, reps, per):
    """[s[:per]] * reps + [s[per:]] along axis 0: B from S, and the prediction of every periodic output from the model's."""
    tail = s.shape[0] - per
    assert tail >= 0
    rest = tuple(s.shape[1:])
    if _torch(s):
        import torch
        b = torch.empty((reps * per + tail,) + rest, dtype=s.dtype, device=s.device)
        if per:
            b[:reps * per].view((reps, per) + rest).copy_(s[:per].unsqueeze(0).expand((reps, per) + rest))
        b[reps * per:] = s[per:]
        return b
    return np.concatenate([s[:per]] * reps + [s[per:]], axis=0)


def periodic(b, s, reps, per):
    """b == expand(s, reps, per) bit for bit, without building the right-hand side."""
    if b.shape[0] != reps * per + s.shape[0] - per or tuple(b.shape[1:]) != tuple(s.shape[1:]):
        return False
    b, s = bits(b), bits(s)
    if not same(b[reps * per:], s[per:]):
        return False
    if per == 0:
        return True
    rest = tuple(s.shape[1:])
    if _torch(b):
        import torch
        return bool(torch.equal(b[:reps * per].view((reps, per) + rest), s[:per].unsqueeze(0).expand((reps, per) + rest)))
    return bool((b[:reps * per].reshape((reps, per) + rest) == s[:per][None]).all())


def _u32(a):
    """Counts held in 32 bits (the library's tables are uint32; torch shows them as int32) as int64."""
    if _torch(a):
        import torch
        return a.to(torch.int64) & 0xFFFFFFFF
    return np.asarray(a).astype(np.int64) & 0xFFFFFFFF


def expand_counted(s, reps, per, step):
    """A table of running counts (one entry per tile and the total): period k repeats the model's first `per` entries plus
    k * step, the tail follows on (reps - 1) * step."""
    s = np.asarray(_u32(s) if not _torch(s) else _u32(s).cpu().numpy())
    k = np.repeat(np.arange(reps, dtype=np.int64), per) * step
    return np.concatenate([np.tile(s[:per], reps) + k, s[per:] + (reps - 1) * step])


def counted(b, s, reps, per, step):
    if b.shape[0] != reps * per + s.shape[0] - per:
        return False
    b, s = _u32(b), _u32(s)
    if _torch(b):
        import torch
        k = torch.arange(reps, dtype=torch.int64, device=b.device).unsqueeze(1) * int(step)
        return bool(torch.equal(b[:reps * per].view(reps, per), s[:per].unsqueeze(0) + k)) and \
            bool(torch.equal(b[reps * per:], s[per:] + (reps - 1) * int(step)))
    return bool(np.array_equal(b, expand_counted(s, reps, per, step)))


def _host(a):
    return a.cpu().numpy() if _torch(a) else np.asarray(a)


# ---- one predictor per output kind: the big array's output against the model's ----
def period_counts(bin_s, w):
    """(exact coefficients of one period, of the tail) from the model's bin ids."""
    b = _host(bin_s)[:w.model_stream_n]
    fl = b == 255
    fl[::BLK] = False                                               # the DC slot is no exact coefficient
    return int(fl[:w.stream_per].sum()), int(fl[w.stream_per:].sum())


def streams_ok(w, out_b, cnt_b, out_s, cnt_s):
    """bin ids, DC and AC_exact of the big array are the model's, period after period; the count is reps * P + tail."""
    cp, ct = period_counts(out_s["bin_index"], w)
    if cp + ct != cnt_s or cnt_b != w.reps * cp + ct:
        return False
    nb_b, nb_s = -(-w.stream_n // BLK), -(-w.model_stream_n // BLK)
    return (periodic(out_b["bin_index"][:w.stream_n], out_s["bin_index"][:w.model_stream_n], w.reps, w.stream_per)
            and periodic(out_b["dc"][:nb_b], out_s["dc"][:nb_s], w.reps, w.stream_per // BLK)
            and periodic(out_b["ac_exact"][:cnt_b], out_s["ac_exact"][:cnt_s], w.reps, cp))


def decode_ok(w, rec_b, rec_s):
    """Any output with the array's own geometry: the decode, the filled copy."""
    return tuple(rec_b.shape) == w.shape and tuple(rec_s.shape) == w.model_shape and periodic(rec_b, rec_s, w.reps, w.period)


def index_ok(w, idx_b, idx_s, cp):
    """idx[k tiles_per + i] = k cnt_P + idx_S[i]; the last entry is the total."""
    return idx_b.shape[0] == w.tiles + 1 and counted(idx_b, idx_s, w.reps, w.tiles_per, cp)


def records_ok(w, recs_b, recs_s):
    """Summary records, (tiles, 8)."""
    return recs_b.shape[0] == w.tiles and periodic(recs_b, recs_s, w.reps, w.tiles_per)


def fix_ok(w, fix_b, fix_s):
    """The correction list (fix_start, fix_off, fix_val, count); fix_off / fix_val None: the count-only form."""
    sb, ob, vb, kb = fix_b
    ss, os_, vs, ks = fix_s
    cp = int(_host(_u32(ss))[w.tiles_per])
    if kb != w.reps * cp + (ks - cp) or sb.shape[0] != w.tiles + 1 or not counted(sb, ss, w.reps, w.tiles_per, cp):
        return False
    if ob is None:
        return vb is None
    return periodic(ob[:kb], os_[:ks], w.reps, cp) and periodic(vb[:kb], vs[:ks], w.reps, cp)


def mask_ok(w, mask_b, count_b, mask_s, count_s):
    """Mask words (one per 64 elements in C order) and the count of missing elements."""
    words_b, words_s = -(-w.n // BLK), -(-(w.elem_per + w.tail * w.row) // BLK)
    if mask_b.shape[0] != words_b or mask_s.shape[0] != words_s:
        return False
    m = _host(mask_s).view(np.uint64)
    mp = int(np.unpackbits(m[:w.elem_per // BLK].view(np.uint8)).sum())
    mt = int(np.unpackbits(m[w.elem_per // BLK:].view(np.uint8)).sum())
    return mp + mt == count_s and count_b == w.reps * mp + mt and periodic(mask_b, mask_s, w.reps, w.elem_per // BLK)


def probe_counts(w, cnt_p, cnt_s):
    """Per bound: reps * cnt_P + cnt_tail, cnt_P from probing P alone, cnt_tail = cnt_S - cnt_P.  Sums of squares combine
    the same way."""
    return [w.reps * p + (s - p) for p, s in zip(cnt_p, cnt_s)]


def probe_ok(w, cnt_b, cnt_p, cnt_s):
    return [int(v) for v in cnt_b] == [int(v) for v in probe_counts(w, cnt_p, cnt_s)]


# ---- patterns ----
def pattern(w, kind="ragged"):
    """One period of workload w (numpy, fp64): `ragged` smooth + noise with a few exact coefficients in a hundred (sf = 10);
    `smooth` / `noisy` the coarse-decode file's fields (sf = 100); `holes` mask_cases' smooth data with blobs of 1e36, Inf and
    NaN markers and the special values that stay valid (sf = 1 once filled)."""
    from tests import mask_cases as M
    from tests import workloads as W
    n = w.elem_per
    if kind == "ragged":
        p = W.ragged(n, np.float64, scale=37.0)
    elif kind in ("smooth", "noisy"):
        i = np.arange(n, dtype=np.float64)
        p = 100.0 + 60.0 * np.sin(i / 4000.0) + 6.0 * np.cos(i / 1000.0)
        if kind == "noisy":
            p = p + 25.0 * np.clip(np.random.default_rng(n).standard_normal(n), -4.0, 4.0)
    elif kind == "holes":
        p = M.build_input(n, np.float64, "blobs", "nan_inf_abs_ge")[0]
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(p.reshape((w.period,) + w.rest))


HOLES = ("nan_inf_abs_ge",)             # mask_cases.RULES key of the `holes` pattern


def model(w, p):
    """S = [P | tail], the tail a prefix of P."""
    assert p.shape == (w.period,) + w.rest
    return np.ascontiguousarray(np.concatenate([p, p[:w.tail]], axis=0))


def shifted(w, s):
    """The negative control: B with everything from its last period on shifted by one block (flat: 64 elements; tiled: one
    block edge along axis 0) of the periodic extension.  It still holds every value of P, so sf is unchanged."""
    b = expand(s, w.reps, w.period)
    step = EDGE[len(w.shape)] if w.tiled else BLK
    at = (w.reps - 1) * w.period
    ext = np.concatenate([s[:w.period]] * 3, axis=0)
    b[at:] = ext[step:step + b.shape[0] - at]
    return b


# ---- the flat correction list restated (tests/test_gpu_fixup.py: Streams.expect) ----
def flat_fix_list(x, r, bound):
    """(fix_start uint32[tiles + 1], fix_off uint16[count], fix_val[count], count): every i with not |x[i] - r[i]| <= bound."""
    with np.errstate(invalid="ignore"):
        m = ~(np.abs(x - r) <= x.dtype.type(bound))
    tiles = -(-x.size // TILE)
    pad = np.zeros(tiles * TILE, bool)
    pad[:x.size] = m
    start = np.concatenate([[0], np.cumsum(pad.reshape(tiles, TILE).sum(axis=1).astype(np.uint64))]).astype(np.uint32)
    at = np.flatnonzero(m)
    return start, (at % TILE).astype(np.uint16), x[at], int(at.size)


def flat_index(bin_index):
    """The exception index restated: idx[t] = exact coefficients in front of element 4096 t, idx[tiles] the total."""
    n = bin_index.size
    fl = bin_index == 255
    fl[::BLK] = False
    tiles = -(-n // TILE)
    pad = np.zeros(tiles * TILE, np.int64)
    pad[:n] = fl
    return np.concatenate([[0], np.cumsum(pad.reshape(tiles, TILE).sum(axis=1))]).astype(np.uint32)
