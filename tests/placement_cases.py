"""Placement ("Placement, what is pinned"): where the caller's buffers start.  The roles include/dctz_hip.h
gives the pointer arguments of every work call, the two placements, and the fixed schedules tests/test_gpu_placement.py plays.
Pure data, numpy and the oracle: nothing here touches a GPU; tests/test_placement_cases_cpu.py holds the census.

A ROLE is the alignment `a` the header gives a buffer: 16, 8, 4, 2, or ES -- the element size of the call's data type.  With it
  PAST    the buffer starts at an address = a (mod 256): aligned to a and to nothing more;
  BEFORE  at 256 - a (mod 256): a buffer at its minimum then straddles every 8-, 16-, 32-, 64- and 128-byte line;
  MIXED   the buffers of one runner alternate between the two (batches: members of both placements in one call).
"""
import ctypes as C

import numpy as np

from dctz_amd import hip as H
from oracle import oracle as O
from tests import sequence_cases as S

LINE = 256
ES, HOST, ANY = "es", "host", "any"      # ES: the element size; HOST: a host pointer; ANY: a device pointer the test itself places
PAST, BEFORE, MIXED = "past", "before", "mixed"
PLACEMENTS = (PAST, BEFORE)

_STREAMS_IN = (16, 4, 4)                 # bin_index, DC, AC_exact as the inputs of a decode-side call
_STREAMS_OUT = (16, 16, 16)              # ... as the outputs of a compress call
_DECODE = _STREAMS_IN + (4, HOST)        # ... with the exception index and the QT table (host memory)

# function -> the roles of its void* arguments behind the context, in order (the prototypes of dctz_amd.hip give the positions)
ROLES = {
    "dctzhip_compress": (16,) + _STREAMS_OUT + (16, 16),                      # d_in; streams; d_scaled, d_coef
    "dctzhip_compress_nd": (16,) + _STREAMS_OUT + (16,),
    "dctzhip_compress_part": (16, 16, 4, 4),                                 # d_in; bin_index + lo, DC + lo / 64, AC_exact + ac_at
    "dctzhip_decompress": _STREAMS_IN + (HOST, 16),
    "dctzhip_decompress_nd": _STREAMS_IN + (HOST, 16),
    "dctzhip_ac_index": (16, 4),
    "dctzhip_decompress_range": _DECODE + (16,),
    "dctzhip_decompress_box": _DECODE + (16,),
    "dctzhip_decompress_box_nd": _DECODE + (16,),
    "dctzhip_decompress_boxes": _DECODE + (HOST,),                           # (the item table; its d_out: TABLES)
    "dctzhip_decompress_boxes_nd": _DECODE + (HOST,),
    "dctzhip_decompress_coarse": _DECODE + (16,),
    "dctzhip_decompress_coarse_nd": _DECODE + (16,),
    "dctzhip_decompress_coarse_box_nd": _DECODE + (16,),
    "dctzhip_decompress_coarse_boxes_nd": _DECODE + (HOST,),
    "dctzhip_tile_summary": _DECODE + (16, 8),                               # d_ref, d_tiles
    "dctzhip_tile_summary_nd": _DECODE + (ES, 8),
    "dctzhip_fixup_build": _DECODE + (16, 4, 2, ES),                         # d_ref, fix_start, fix_off, fix_val
    "dctzhip_fixup_build_nd": _DECODE + (16, 4, 2, ES),
    "dctzhip_fixup_apply": (4, 2, ES, ES),                                   # fix_start, fix_off, fix_val, d_out
    "dctzhip_fixup_apply_nd": (4, 2, ES, ES),
    "dctzhip_mask_build": (16, 8, 16),                                       # d_in, d_mask, d_filled
    "dctzhip_mask_build_nd": (16, 8, 16),
    "dctzhip_mask_apply": (8, ES),
    "dctzhip_compress_masked": (16,) + _STREAMS_OUT + (8, 16),
    "dctzhip_compress_masked_nd": (16,) + _STREAMS_OUT + (8, 16),
    "dctzhip_dct_blocks": (16, 16),
    "dctzhip_stats": (16,),
    "dctzhip_serial_mean_begin": (16,),                                      # (the header states none: 16)
    "dctzhip_scale_inplace": (16,),
    "dctzhip_psnr_terms": (16, 16),                                          # (the header states none: 16)
    "dctzhip_rd_probe": (16,),
    "dctzhip_rd_probe_nd": (16,),
    "dctzhip_compress_psnr": (16,) + _STREAMS_OUT,
    "dctzhip_compress_psnr_nd": (16,) + _STREAMS_OUT,
}
# host-side item tables: function -> (position of the count, position of the table, the item type, field -> role)
TABLES = {
    "dctzhip_compress_batch": (1, 2, H.BatchCItem, {"d_in": 16, "d_bin_index": 16, "d_dc": 16, "d_ac_exact": 16, "d_scaled": 16}),
    "dctzhip_decompress_batch": (1, 2, H.BatchDItem, {"d_bin_index": 16, "d_dc": 4, "d_ac_exact": 4, "d_out": 16}),
    "dctzhip_decompress_boxes": (14, 15, H.BoxItem, {"d_out": 16}),
    "dctzhip_decompress_boxes_nd": (13, 14, H.BoxItem, {"d_out": 16}),
    "dctzhip_decompress_coarse_boxes_nd": (14, 15, H.BoxItem, {"d_out": 16}),
}
# work calls whose device pointers are NOT held to a placement, each with its reason
ALLOW = {
    "dctzhip_deflate_ex": "byte sections: the header asks no alignment of them (4 bytes give the fast load path); the sources are "
                          "the decode slots as they stand, the outputs the wrapper's own allocations (torch, not Context.torch)",
    "dctzhip_inflate": "as dctzhip_deflate_ex",
    "dctzhip_deflate": "the refused call of 9 sections only; not in the placement schedules",
}
# kind -> the work calls it makes (what the proxy must have seen when the op returns)
KIND_CALLS = {
    "compress": ["dctzhip_compress"], "compress_scaled": ["dctzhip_compress"], "compress_inplace": ["dctzhip_compress"],
    "compress_coef": ["dctzhip_compress"], "dct_blocks": ["dctzhip_dct_blocks"], "decompress": ["dctzhip_decompress"],
    "compress_nd": ["dctzhip_compress_nd"], "decompress_nd": ["dctzhip_decompress_nd"],
    "range": ["dctzhip_ac_index", "dctzhip_decompress_range"], "box": ["dctzhip_decompress_box"], "boxes": ["dctzhip_decompress_boxes"],
    "box_nd": ["dctzhip_decompress_box_nd"], "boxes_nd": ["dctzhip_decompress_boxes_nd"],
    "coarse": ["dctzhip_decompress_coarse"], "coarse_nd": ["dctzhip_decompress_coarse_nd"],
    "coarse_box_nd": ["dctzhip_decompress_coarse_box_nd"], "coarse_boxes_nd": ["dctzhip_decompress_coarse_boxes_nd"],
    "summary": ["dctzhip_tile_summary"], "summary_ref": ["dctzhip_tile_summary"],
    "summary_nd": ["dctzhip_tile_summary_nd"], "summary_nd_ref": ["dctzhip_tile_summary_nd"],
    "fixup_count": ["dctzhip_fixup_build"], "fixup_list": ["dctzhip_fixup_build"], "fixup_apply": ["dctzhip_fixup_apply"],
    "fixup_count_nd": ["dctzhip_fixup_build_nd"], "fixup_list_nd": ["dctzhip_fixup_build_nd"], "fixup_apply_nd": ["dctzhip_fixup_apply_nd"],
    "mask_build": ["dctzhip_mask_build"], "mask_build_nd": ["dctzhip_mask_build_nd"],
    "compress_masked": ["dctzhip_compress_masked"], "compress_masked_nd": ["dctzhip_compress_masked_nd"], "mask_apply": ["dctzhip_mask_apply"],
    "rd_probe": ["dctzhip_rd_probe"], "rd_probe_nd": ["dctzhip_rd_probe_nd"],
    "compress_psnr": ["dctzhip_compress_psnr"], "compress_psnr_nd": ["dctzhip_compress_psnr_nd"], "psnr_terms": ["dctzhip_psnr_terms"],
    "compress_batch": ["dctzhip_compress_batch"], "decompress_batch": ["dctzhip_decompress_batch"],
    "deflate": ["dctzhip_deflate_ex"], "inflate": ["dctzhip_inflate"],
}


def pointer_positions(func):
    """The positions of the void* arguments of `func` behind the context."""
    return [i for i, t in enumerate(H._PROTOS[func][1]) if t is C.c_void_p and i > 0]


def alignment(role, esize):
    return int(esize) if role == ES else int(role)


def residue(role, esize, placement):
    """The address (mod 256) of a buffer of `role` under `placement`."""
    a = alignment(role, esize)
    assert placement in PLACEMENTS and 0 < a < LINE and LINE % a == 0
    return a if placement == PAST else LINE - a


def alloc_role(kind, dtype_name):
    """The role of a buffer the runner or the wrapper allocates during an op of `kind` without naming one, from its element
    type ("uint8", "int16", "int32", "int64", "float32", "float64").  Everything the rule cannot tell is 16."""
    if kind.startswith("summary"):
        return 8                                           # the records (float64 x 8 per tile)
    if kind.startswith("fixup_count") or kind.startswith("fixup_list"):
        return {"int32": 4, "int16": 2, "float32": ES, "float64": ES}.get(dtype_name, 16)      # fix_start, fix_off, fix_val
    if kind in ("mask_build", "mask_build_nd", "compress_masked", "compress_masked_nd") and dtype_name == "int64":
        return 8                                           # the mask words
    if kind == "range" and dtype_name == "int32":
        return 4                                           # the index dctzhip_ac_index writes
    return 16


# ---- the schedules: a fixed order, no random walk -------------------------------------------------------------------------------
E2_FLAT = ("a91", "a2597", "b12325", "c12288")            # E2 kinds, flat: both element types, short blocks of 27 and 37, whole tiles
SPEC_SUBJECTS = ("big", "big32")
KNOB_FAMILIES = ("compress", "decompress")                 # ... also on the chain, and on the chain with the split kernel


def _subjects(kind):
    names = [n for n in S.SUBJECTS if S.applies(kind, n)]
    if S.OPS[kind][3] == S.E2:
        names = [n for n in names if not S.SUBJECTS[n].flat or n in E2_FLAT]
    return names


def _pass(family, rng, only=None):
    ops = []
    for kind in S.KINDS_OF[family]:
        for name in _subjects(kind):
            if only is None or name in only:
                ops.append((kind, name, S.make_args(kind, name, rng)))
    return ops


def schedule(family):
    """Every kind of `family` on every subject it applies to (E2 kinds: on one subject at least per element type and geometry);
    compress and decompress also with set_one_launch(off) and then set_split(on), `big` / `big32` with the sampled guess of sf."""
    rng = np.random.default_rng(4242 + S.FAMILIES.index(family))
    if family == "batch":
        ops = []
        for mode in (O.EC, O.QT):
            for _ in range(2):
                m = S.batch_members(rng, mode)
                ops += [("compress_batch", m[0], {"members": m}), ("decompress_batch", m[0], {"members": m})]
        return ops
    ops = _pass(family, rng)
    if family in KNOB_FAMILIES:
        ops += [S.op("spec_on")] + _pass(family, rng, SPEC_SUBJECTS)
        ops += [S.op("one_off")] + _pass(family, rng)
        ops += [S.op("split_on")] + _pass(family, rng)
    return ops


def schedules():
    return {f: schedule(f) for f in S.FAMILIES}


RAW_SUBJECTS = ("a2597", "c12288")                         # compress_part, stats, scale_inplace and the serial mean: once each


def census(scheds):
    """kind -> the element types it ran on."""
    seen = {k: set() for k in S.OPS}
    for sched in scheds:
        for kind, name, args in sched:
            if kind in S.OPS:
                for t in S.targets(kind, name, args):
                    seen[kind].add(S.SUBJECTS[t].dtype)
    return seen
