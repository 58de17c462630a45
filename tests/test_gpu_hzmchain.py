"""wtz_set_window_chaining(ctx, 0) on the MI355X (K_pair_chain: the windows of a scan by chaining_hzmps, hzm_aln.h:351-408, 544-561): the vectors recorded from
the reference's own compiled align_hzmaux with HZM_FAST_WINDOW_KMER_CHAINING = 0 (tests/golden/hzmchain_vectors.npz, 101 calls on ten backbones), through the
one-call service and through the stage-level path with the window boxes - one context per parameter set (O = -3, O = -2: a context has one), every backbone and
read of the set in it, one call; and one pair whose first scan holds more matches than the LDS slice takes, so that the chain's nodes live in the pool workspace,
against the same task bodies run with one lane (the host emulation).  What is and is not pinned: tests/test_hzmchain_cpu.py."""
import os
import subprocess

import pytest

import hzmchainvec as cv
import hzmregvec as hv
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emul_lib():
    subprocess.run([os.path.join(ROOT, "tests", "emul", "build_emul.sh")], check=True)
    return os.path.join(ROOT, "tests", "emul", "libwtz_emul.so")


def test_recorded_vectors():
    assert cv.check_vectors(None, cv.load_vectors()) >= 2 * 90


def test_chain_in_the_pool_workspace_equals_the_emulation(emul_lib):
    """1 455 matches in the first scan (by the model of the reference's walk; 257 are the least that cannot fit 8 KiB): the scan's workspace, and with it the
    chain's nodes, is in the pool.  Service and stage path, chain form and - the same scan body around another per-window block - the fast form."""
    prm = cv.load_vectors()[0]["prm"]
    G, rd, beg, end = cv.dense_window_pair()
    assert cv.first_scan_matches(G, rd, prm, beg, end) >= 257
    got = {}
    for lib in (emul_lib, None):
        ctx = hv.open_ctx(lib, [G, rd], prm=prm, min_sm=0.5)
        try:
            for fast in (0, 1):
                ctx.set_window_chaining(fast)
                svc = hv.service(ctx, [0], [1], [beg], [end])
                stg, wins = cv.stages_with_windows(ctx, [G.size, rd.size], [0], [1], [beg], [end], 0.5)
                assert svc[0] is not None and cv.equal(svc[0], stg[0]) and wins[0] is not None
                got[lib, fast] = (svc[0], wins[0].tolist())
        finally:
            ctx.close()
    for fast in (0, 1):
        dev, emu = got[None, fast], got[emul_lib, fast]
        assert cv.equal(dev[0], emu[0]) and dev[1] == emu[1], "fast = %d: device %s / %s, emulation %s / %s" % (fast, dev[0][0], dev[1], emu[0][0], emu[1])
    assert not cv.equal(got[None, 0][0], got[None, 1][0]), "the two forms agree on this pair: the case shows nothing"
