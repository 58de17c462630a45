"""The k-mer index and the seed lookup (index_wtzmo, query_wtzmo: wtzmo.c:349-573) function by function, on the CPU: the oracle's restatement and the host
emulation of the device library against the recorded answers of the reference's own functions (tests/golden/seed_vectors.npz, tests/seedvec.py), the
regimes each case is there for asserted on those answers, and - where oracle/_ref/libref_seed.so is built - the reference called live."""
import os

import numpy as np
import pytest

import seedvec as sv

VARIANTS = sv.variants()
IDS = ["%s-%s" % v for v in VARIANTS]


@pytest.fixture(scope="module")
def oracle():
    return sv.oracle_lib()


def test_regimes_hold_on_the_recorded_reference_data():
    """every case's regime, against the constants of the DEVICE build of wtz_seed.h (not the emulation's small ones)"""
    K = sv.constants()
    assert K["WTZ_CWG_L2_MIN"] == 2 * K["WTZ_CWG_CAP"] and K["WTZ_CWG_SKETCH"] == 65536
    lines = sv.check_regimes(sv.load_record, VARIANTS, {c: sv.checked_reads(c) for c in sv.READS})
    print("\n".join(lines))
    assert len(lines) >= 12


def test_no_read_length_separates_the_double_multiply_from_the_integer_one():
    """wtzmo.c:445 multiplies by 1.2 in double; below 10 kb (and up to the 24 bits of rdlen) that equals L * 6 / 5, so the length gate needs no special L"""
    assert all(int(L * 1.2) == L * 6 // 5 for L in range(10000))
    assert all(int(np.uint32(L) * 1.2) == L * 6 // 5 for L in range(5, 1 << 24, 4999))


def test_the_fixture_covers_every_case_and_stays_small():
    have = {c for c, _ in VARIANTS}
    assert have == set(sv.READS), have ^ set(sv.READS)
    assert {t for c, t in VARIANTS if c == "plain"} >= {"default", "S1", "k5", "k32", "k15", "k17", "H0", "d1", "d255", "d256", "d5000", "A1", "A2", "A5", "K2", "K3"}
    assert os.path.getsize(sv.NPZ) < 300 * 1000
    assert set(sv.PARTS) == {"halves", "thirds"}


@pytest.mark.parametrize("case,tag", VARIANTS, ids=IDS)
def test_oracle_equals_the_recorded_reference(oracle, case, tag):
    """every group (key, ol, cnt) in merge order, the heap arrays verbatim, the statistics and the (k-mer, count) table"""
    var, rec = sv.load_record(case, tag)
    got = sv.run_seedx(oracle, sv.checked_reads(case), var)
    sv.compare_record(rec, got, var["prm"]["kovl"], "oracle %s/%s" % (case, tag), full=True)
    assert got["max_cnt"] == rec["max_cnt"]


@pytest.mark.parametrize("name", sorted(sv.PARTS))
def test_oracle_parts_equal_the_reference_called_part_by_part(oracle, name):
    var, _ = sv.load_record("plain", "default")
    var["queries"] = None
    got = sv.run_seedx_parts(oracle, sv.checked_reads("plain"), var, sv.PARTS[name])
    for q, (w, g) in enumerate(zip(sv.load_parts(name), got)):
        sv.compare_rows(w, g, q, "oracle parts " + name)


@pytest.mark.parametrize("case,tag", VARIANTS, ids=IDS)
def test_emulation_equals_the_recorded_reference(case, tag):
    """the device library's code as host loops: wtz_index_build, wtz_index_count / _counts_fetch / _finish, wtz_candidate_groups_*, wtz_candidates.  The two
    cases with half a million listed tuples run on the emulation built with the device's second-level thresholds (thousands of parts under its own)."""
    var, rec = sv.load_record(case, tag)
    got = sv.run_device(sv.emul_lib(device_thresholds=(case, tag) in sv.HEAVY), sv.checked_reads(case), var)
    sv.compare_record(rec, got, var["prm"]["kovl"], "emulation %s/%s" % (case, tag))
    assert got["n_kept_finish"] == rec["stats"]["n_kept"]


@pytest.mark.parametrize("case,tag", [("fat_group", "S1"), ("many_reads", "default"), ("plain", "default"), ("strand_merge", "S1")])
def test_emulation_with_device_thresholds_equals_the_recorded_reference(case, tag):
    """the same code with WTZ_CWG_L2_MIN and WTZ_CWG_L2_PART_UNITS as the device has them: the second level entered (or not) where the device enters it"""
    var, rec = sv.load_record(case, tag)
    got = sv.run_device(sv.emul_lib(device_thresholds=True), sv.checked_reads(case), var)
    sv.compare_record(rec, got, var["prm"]["kovl"], "emulation (device thresholds) %s/%s" % (case, tag))


@pytest.mark.parametrize("name", sorted(sv.PARTS))
def test_emulation_parts_and_shards(name):
    """parts equal the reference called part by part; shards equal the UNSHARDED reference"""
    var, rec = sv.load_record("plain", "default")
    seqs = sv.checked_reads("plain")
    got = sv.run_device_parts(sv.emul_lib(), seqs, var, sv.PARTS[name])
    for q, (w, g) in enumerate(zip(sv.load_parts(name), got)):
        sv.compare_rows(w, g, q, "emulation parts " + name)
    st, sha, groups, rows = sv.run_device_shards(sv.emul_lib(), seqs, var, sv.PARTS[name])
    sv.compare_stats(rec["stats"], dict(st, avg_rdlen=rec["stats"]["avg_rdlen"]), "emulation shards " + name)
    assert bytes(sha) == bytes(rec["tab_sha"])
    for i, q in enumerate(rec["q"]):
        sv.compare_groups(rec["groups"][i], groups[q], var["prm"]["kovl"], q, "emulation shards " + name)
        sv.compare_rows(rec["rows"][i], rows[q], q, "emulation shards " + name)


# ---- the reference called live ----
live = pytest.mark.skipif(not os.path.exists(sv.SHIM), reason="reference seed shim not built (needs the reference's sources once)")


@live
def test_recorded_vectors_are_what_the_reference_answers_now():
    ref = sv.SeedLib(sv.SHIM)
    for case, tag in (("plain", "default"), ("short", "S1"), ("fat_group", "S1")):
        var, rec = sv.load_record(case, tag)
        sv.compare_record(rec, sv.run_seedx(ref, sv.checked_reads(case), var), var["prm"]["kovl"], "reference %s/%s" % (case, tag), full=True)


@live
@pytest.mark.parametrize("shape", ["plain", "heap", "strand_merge"])
def test_oracle_and_emulation_equal_the_live_reference_on_fresh_seeds(oracle, shape):
    """20 seeds per shape; heap = the plain shape with -A 2"""
    ref = sv.SeedLib(sv.SHIM)
    emul = sv.emul_lib()
    for seed in range(100, 120):
        seqs = sv.strand_reads(seed) if shape == "strand_merge" else sv.plain_reads(seed)
        var = sv.V(ksave=1) if shape == "strand_merge" else sv.V(ncand=2) if shape == "heap" else sv.V()
        want = sv.run_seedx(ref, seqs, var)
        where = "%s seed %d" % (shape, seed)
        sv.compare_record(want, sv.run_seedx(oracle, seqs, var), var["prm"]["kovl"], "oracle " + where, full=True)
        sv.compare_record(want, sv.run_device(emul, seqs, var), var["prm"]["kovl"], "emulation " + where)
