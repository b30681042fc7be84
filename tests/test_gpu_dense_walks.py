"""
The three dense walks -- ms_scan_best, ms_scan_affinity, ms_scan_score_histogram -- on ONE world in which their three plans differ, held
against each other by exact identities.  The walks share the host's plan (ms_dense_plan.h), its upload and the launch loops; here the
plans differ in which motifs are walked and in where the tiles break:

    motif                      best              affinity          histogram
    0  width 5                 tile 0            tile 0            tile 0
    1  width 33                tile 0            tile 0            tile 0
    2  a NaN entry             skipped           skipped           skipped
    3  every entry <= 0        skipped           tile 1            skipped         (max_raw <= 0)
    4  width Wh                tile 1            tile 1            tile 1          (Wh: the histogram's widest tiled motif)
    5  width Wh + 1            tile 2            tile 2            table in HBM
    6  width Wa                tile 3            tile 3            table in HBM    (Wa: the widest tiled motif of the other two)
    7  width Wa + 1            table in HBM      table in HBM      table in HBM

Regions of 0, 4, seg, seg + 1 and 2 seg + 17 bases and one of seg + 1 with a few N: one segment and more, with and without partials.
Both strands, max_n = -1, one count per (window, strand), lo / hi wide enough that no count falls outside the bins.  Every scan runs
twice when the module's first test asks for the world; the tests share the results.
"""
import numpy as np
import pytest

from motifscan_amd import _lib

pytestmark = pytest.mark.gpu

N_BINS, LO, HI = 64, -4096.0, 4096.0
NAN_MOTIF, NEG_MOTIF = 2, 3


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


class World:
    def __init__(self):
        rng = np.random.default_rng(20241020)
        seg, wa, wh = _lib.best_segment_windows(), _lib.affinity_dims()["tile_max_width"], _lib.scorehist_dims()["tile_max_width"]
        assert _lib.affinity_dims()["segment_windows"] == seg and _lib.scorehist_dims()["segment_windows"] == seg and wh + 1 < wa

        def mat(width):                                  # (raw sums of a thousand columns stay within a few units)
            return np.round(rng.normal(0.0, 1.2, size=(4, width)), 3) * (0.05 if width > 64 else 1.0)

        holed = mat(7)
        holed[2, 3] = np.nan
        self.mats = [mat(5), mat(33), holed, -np.abs(mat(6)) - 0.001, mat(wh), mat(wh + 1), mat(wa), mat(wa + 1)]
        self.widths = [m.shape[1] for m in self.mats]

        def seq(length):
            return "".join(rng.choice(list("ACGT"), size=length)) if length else ""

        with_n = list(seq(seg + 1))
        for at in (0, 31, 32, seg // 2, seg):
            with_n[at] = "N"
        self.seqs = [seq(0), seq(4), seq(seg), seq(seg + 1), seq(2 * seg + 17), "".join(with_n)]
        self.lengths = np.array([len(s) for s in self.seqs])

        pw, sq = _lib.PwmSet.from_matrices(self.mats), _lib.SeqSet.from_strings(self.seqs)
        try:
            self.max_raw = np.asarray(pw.max_raw())
            self.best, self.aff, self.hist = [], [], []
            for _ in range(2):
                res = _lib.scan_best(pw, sq, 3)
                try:
                    assert res.shape == (len(self.mats), len(self.seqs))
                    self.best.append(res.sites())
                finally:
                    res.close()
                res = _lib.scan_affinity(pw, sq, 3, 1.0, -1)
                try:
                    assert res.shape == (len(self.mats), len(self.seqs))
                    self.aff.append(res.cells())         # (peak, sum, n_terms, log_mean)
                finally:
                    res.close()
                self.hist.append(_lib.score_histogram(pw, sq, 3, LO, HI, N_BINS))
        finally:
            sq.close()
            pw.close()
        self.best_scores = [m for m in range(len(self.mats)) if m not in (NAN_MOTIF, NEG_MOTIF)]
        assert all(np.isfinite(self.max_raw[m]) and self.max_raw[m] > 0 for m in self.best_scores)
        assert self.max_raw[NEG_MOTIF] <= 0


@pytest.fixture(scope="module")
def world():
    return World()


def test_peak_over_max_raw_is_the_best_site_score_and_a_term_is_a_winner(world):
    (score, pos, strand), (peak, _, n_terms, _) = world.best[0], world.aff[0]
    checked = 0
    for m in world.best_scores:
        want = peak[m] / world.max_raw[m]                # no entry is -inf: a cell with a term has a finite peak
        assert np.array_equal(np.isnan(score[m]), np.isnan(want))
        ok = ~np.isnan(want)
        assert score[m][ok].tobytes() == want[ok].tobytes()
        assert np.array_equal(pos[m] >= 0, n_terms[m] > 0)
        assert np.array_equal(strand[m] != 0, n_terms[m] > 0)
        windows = np.maximum(world.lengths - world.widths[m] + 1, 0)
        assert np.array_equal(n_terms[m], 2 * windows)   # both strands, no window dropped
        checked += int(ok.sum())
    assert checked == sum(int((world.lengths >= world.widths[m]).sum()) for m in world.best_scores) >= 12      # every cell that holds a window


def test_histogram_rows_count_the_terms(world):
    hist, n_terms = world.hist[0], world.aff[0][2]
    assert hist.shape == (len(world.mats), N_BINS + 2)
    for m in range(len(world.mats)):
        if m in world.best_scores:
            assert int(hist[m].sum()) == int(n_terms[m].astype(np.int64).sum()) > 0
            assert hist[m, 0] == 0 and hist[m, N_BINS + 1] == 0
        else:
            assert int(hist[m].sum()) == 0
    assert int(n_terms[NEG_MOTIF].sum()) > 0             # affinity alone walks the motif whose max_raw is <= 0


def test_rows_of_skipped_motifs_are_the_documented_fills(world):
    (score, pos, strand), (peak, total, n_terms, log_mean), hist = world.best[0], world.aff[0], world.hist[0]
    for m in (NAN_MOTIF, NEG_MOTIF):                     # "no winner"
        assert np.isnan(score[m]).all() and (pos[m] == -1).all() and (strand[m] == 0).all()
        assert not hist[m].any()
    m = NAN_MOTIF                                        # "no term"
    assert (n_terms[m] == 0).all() and np.isnan(peak[m]).all() and (total[m] == 0).all() and np.isnan(log_mean[m]).all()
    assert np.isfinite(peak[NEG_MOTIF][world.lengths >= world.widths[NEG_MOTIF]]).all()


def test_a_second_call_returns_the_same_bytes(world):
    for first, second in zip(list(world.best[0]) + list(world.aff[0]), list(world.best[1]) + list(world.aff[1])):
        assert first.dtype == second.dtype and first.shape == second.shape and first.tobytes() == second.tobytes()
    assert world.hist[0].tobytes() == world.hist[1].tobytes()
