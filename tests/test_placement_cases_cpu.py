"""The census of tests/placement_cases.py: what tests/test_gpu_placement.py plays, the role table against the prototypes of
dctz_amd.hip, and the two placements.  No GPU."""
import ctypes as C

from dctz_amd import hip as H
from tests import placement_cases as P
from tests import sequence_cases as S


def test_every_kind_runs_under_both_placements_on_every_element_type_it_applies_to():
    d = P.schedules()
    assert list(d) == list(S.FAMILIES) and P.PLACEMENTS == ("past", "before")        # (the GPU test plays every schedule under both)
    seen = P.census(d.values())
    assert set(seen) == set(S.OPS)
    for kind, dtypes in seen.items():
        want = {S.SUBJECTS[n].dtype for n in S.SUBJECTS if S.applies(kind, n)}
        assert dtypes == want and want, (kind, dtypes, want)
    for fam, sched in d.items():
        assert S.census([sched])["inapplicable"] == 0, fam
        assert {k for k, _, _ in sched if k in S.OPS} == set(S.KINDS_OF[fam]), fam
        assert all(k in S.OPS or k in S.STATE_OPS for k, _, _ in sched), fam
    assert P.schedules() == P.schedules()
    print("placement census: ops per family", {f: len(v) for f, v in d.items()})


def test_e1_kinds_run_on_every_subject_and_e2_kinds_on_every_geometry_and_type():
    d = P.schedules()
    for kind, (fam, _, _, source) in S.OPS.items():
        if fam == "batch":
            continue
        names = {n for k, n, _ in d[fam] if k == kind}
        every = {n for n in S.SUBJECTS if S.applies(kind, n)}
        if source == S.E1:
            assert names == every, (kind, every - names)
        else:
            geo = lambda n: (S.SUBJECTS[n].dtype, len(S.SUBJECTS[n].shape))              # noqa: E731
            assert {geo(n) for n in names} == {geo(n) for n in every}, kind
    members = {m for k, _, a in d["batch"] for m in a["members"]}
    assert {S.SUBJECTS[m].dtype for m in members} == {S.F32, S.F64} and {S.SUBJECTS[m].mode for m in members} == {0, 1}


def test_knob_passes():
    d = P.schedules()
    for fam in P.KNOB_FAMILIES:
        knobs = [k for k, _, _ in d[fam] if k in S.STATE_OPS]
        assert knobs == ["spec_on", "one_off", "split_on"], fam
        c = S.census([d[fam]])
        role = 0 if fam == "compress" else 1
        assert c["knobs"][("one", 0)][role] > 0 and c["knobs"][("split", 1)][role] > 0 and c["knobs"][("one", 1)][role] > 0
        i, j = [n for n, (k, _, _) in enumerate(d[fam]) if k in ("spec_on", "one_off")]
        assert {n for _, n, _ in d[fam][i + 1:j]} == set(P.SPEC_SUBJECTS)
    assert all(S.SUBJECTS[n].n >= S.SPEC_MIN for n in P.SPEC_SUBJECTS)


def test_role_table_matches_the_prototypes():
    for func, roles in P.ROLES.items():
        assert len(P.pointer_positions(func)) == len(roles), func
        assert all(r in (16, 8, 4, 2, P.ES, P.HOST) for r in roles), func
    for func, (at_k, at_items, item, fields) in P.TABLES.items():
        args = H._PROTOS[func][1]
        assert args[at_k] is C.c_int and (args[at_items] is C.c_void_p or args[at_items]._type_ is item), func
        assert all(dict(item._fields_)[f] is C.c_void_p for f in fields), func
        assert set(fields) == {f for f, t in item._fields_ if t is C.c_void_p and f != "qtable_host"}, func
    # no work call is left out: every function with a void* argument behind the context has its roles, or its reason
    other = {"dctzhip_set_stream", "dctzhip_free", "dctzhip_memcpy_h2d", "dctzhip_memcpy_d2h", "dctzhip_host_register", "dctzhip_host_unregister",
             "dctzhip_comm_unique_id", "dctzhip_comm_create", "dctzhip_comm_gather", "dctzhip_h2d_pipe_begin", "dctzhip_debug_divide"}
    for func, (_, args) in H._PROTOS.items():
        if any(t is C.c_void_p for t in args[1:]) and func not in other:
            assert func in P.ROLES, func
    for func in P.ALLOW:
        assert func not in P.ROLES and P.ALLOW[func]
    # every op has its calls, and every call with roles but the four raw ones belongs to an op
    assert set(P.KIND_CALLS) == set(S.OPS)
    called = {f for fs in P.KIND_CALLS.values() for f in fs}
    raw = {"dctzhip_compress_part", "dctzhip_stats", "dctzhip_serial_mean_begin", "dctzhip_scale_inplace"}
    assert called - set(P.ALLOW) == (set(P.ROLES) | set(P.TABLES)) - raw
    assert set(P.RAW_SUBJECTS) == {"a2597", "c12288"}


def test_residues_and_allocation_rule():
    for role, es in ((16, 4), (8, 8), (4, 4), (2, 2), (P.ES, 4), (P.ES, 8)):
        a = P.alignment(role, es)
        past, before = P.residue(role, es, P.PAST), P.residue(role, es, P.BEFORE)
        assert past == a and before == 256 - a and past % a == 0 and before % a == 0
        assert past % (2 * a) != 0 and before % (2 * a) != 0, "aligned to a and to nothing more"
        # a buffer at its minimum that starts at BEFORE ends on the line: two of them straddle every 8- to 128-byte line
        assert all((before + a) % line == 0 for line in (8, 16, 32, 64, 128) if line >= a)
    assert P.alloc_role("summary_nd", "float64") == 8 and P.alloc_role("fixup_list", "int16") == 2 and P.alloc_role("fixup_list_nd", "float32") == P.ES
    assert P.alloc_role("fixup_count", "int32") == 4 and P.alloc_role("mask_build", "int64") == 8 and P.alloc_role("mask_build", "float64") == 16
    assert P.alloc_role("range", "int32") == 4 and P.alloc_role("compress", "float32") == 16 and P.alloc_role("decompress", "float64") == 16
