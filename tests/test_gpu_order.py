"""
The last step of the hit ordering with region coordinates (ms_order.hip): the radix passes leave runs of hits that agree in the key
bits above L, order_finalize_kernel sorts each run in LDS and writes seq_idx / pos / strand / score, the per-motif offsets and the
per-motif region counts; runs it cannot hold go to order_overflow_kernel.  Every case is compared, bit for bit, with the oracle.

MS_SORT_LOW_BITS forces L (the library otherwise picks it from the expected run length), MS_ORDER_RUN_CAP sends every run longer than
the cap to the overflow path; both are measurement switches, honoured only with MS_MEASURE=1.
"""
import os

import numpy as np
import pytest

from motifscan_amd import _lib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


def _set_env(monkeypatch, low_bits=None, run_cap=None):
    monkeypatch.setenv("MS_MEASURE", "1")
    for name, v in (("MS_SORT_LOW_BITS", low_bits), ("MS_ORDER_RUN_CAP", run_cap)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _region_counts(want, P):
    """regions with >= 1 hit per motif, from the oracle's arrays"""
    off = want["motif_offsets"]
    return np.array([len(np.unique(want["seq_idx"][off[p]:off[p + 1]])) for p in range(P)], dtype=np.int64)


def assert_same(res, want, P):
    got = res.hits()
    assert np.array_equal(got["motif_offsets"], want["motif_offsets"])
    assert np.array_equal(got["seq_idx"], want["seq_idx"])
    assert np.array_equal(got["pos"], want["pos"])
    assert np.array_equal(got["strand"].astype(np.int32), want["strand"].astype(np.int32))
    assert np.array_equal(got["score"], want["score"])          # bit-exact fp64, moved with its key
    assert np.array_equal(np.asarray(res.region_counts(), dtype=np.int64), _region_counts(want, P))


def _word_motif(word, lo=-3.0, hi=1.25):
    m = np.full((4, len(word)), lo)
    for c, b in enumerate(word):
        m["ACGT".index(b), c] = hi
    return m


def _pack(mats, cutoffs):
    vals = np.concatenate([m.ravel() for m in mats])
    widths = np.array([m.shape[1] for m in mats], dtype=np.int32)
    return vals, widths, np.asarray(cutoffs, dtype=np.float64)


def _seqs(seqs):
    raw = "".join(seqs).encode()
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return raw, offsets


@pytest.fixture(scope="module")
def c2(oracle):
    wl = synth.workload("c2")
    vals, widths, cutoffs = wl["pwm_values"], wl["widths"], wl["cutoffs"]
    bases, offsets = wl["sets"][0]
    want = oracle.scan_arrays(vals, widths, cutoffs, bases.tobytes(), offsets, 3, min(50, os.cpu_count() or 1))
    return vals, widths, cutoffs, bases, offsets, want


@pytest.mark.parametrize("low_bits", [8, 16, 24])
def test_c2_config_in_full_at_each_low_bit_count(c2, monkeypatch, low_bits):
    """configs[1] in full with 8, 16 and 24 key bits left to the run sort: at 24 (the whole coordinate of a 10k-region set but its
    top bits) a run is most of one motif's hits, far beyond what LDS holds, so the overflow path orders them."""
    vals, widths, cutoffs, bases, offsets, want = c2
    _set_env(monkeypatch, low_bits=low_bits)
    pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(bases, offsets)
    for _ in range(2):                                          # the exactly-sized form, then the predicted one (padding keys)
        res = _lib.scan(pw, sq, 3)
        assert_same(res, want, len(widths))
        st = res.stats()
        assert st["n_passes"] == 1
        if low_bits == 24:
            assert st["order_overflow_runs"] > 0
        res.close()


def test_default_choice_of_low_bits_and_small_lists(c2, monkeypatch):
    """No switch: the library's own choice of L; MS_SORT_FIXUP_MIN=0: the same on a short list; MS_SORT_FULL: every bit by radix passes
    (L = 0, which keeps finalize_rp_kernel, as lists below the fix-up threshold do)."""
    vals, widths, cutoffs, bases, offsets, want = c2
    for env in ({}, {"MS_SORT_FIXUP_MIN": "0"}, {"MS_SORT_FULL": "1"}):
        _set_env(monkeypatch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(bases, offsets)
        for _ in range(2):
            res = _lib.scan(pw, sq, 3)
            assert_same(res, want, len(widths))
            assert res.stats()["order_overflow_runs"] == 0
            res.close()


def _flood_set():
    rng = np.random.default_rng(5)
    vals, widths, cutoffs = synth.load_motif_set(40, p_value="1e-3")
    mats = [m.copy() for m in synth.matrices_of(vals, widths)]
    cutoffs = list(cutoffs)
    for word in ("AAAAAAAAAA", "ACACACACACAC", "GGCGGCGGC"):       # a hit at nearly every window of a repeat
        mats.append(_word_motif(word))
        cutoffs.append(0.95)
    seqs = ["A" * 40000, "AC" * 3000, "GGC" * 2000, "acgt" * 500]
    seqs += ["".join(rng.choice(list("ACGT"), size=int(n))) for n in rng.integers(9000, 11000, size=58)]
    seqs += ["T" * 5000, "N" * 300 + "A" * 30000]
    # (64 regions of <= 2^16 bases in ~0.7 Mbase: the hit keys carry (region, position), the form this ordering serves)
    return _pack(mats, cutoffs) + _seqs(seqs)


@pytest.mark.parametrize("low_bits,run_cap", [(16, None), (24, None), (8, 4), (16, 1), (None, None)])
def test_runs_longer_than_lds_take_the_overflow_path(oracle, monkeypatch, low_bits, run_cap):
    """Poly-A and dinucleotide / trinucleotide repeats under motifs that hit at nearly every window: runs of tens of thousands of
    hits (a 40 kb homopolymer region), or every run beyond a forced tiny cap.  The overflow path must run and agree, on every strand mode."""
    vals, widths, cutoffs, raw, offsets = _flood_set()
    _set_env(monkeypatch, low_bits=low_bits, run_cap=run_cap)
    pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(raw, offsets)
    for strand in (3, 1, 2):
        want = oracle.scan_arrays(vals, widths, cutoffs, raw, offsets, strand, 8)
        assert len(want["pos"]) > (60000 if strand != 2 else 5000)
        res = _lib.scan(pw, sq, strand)
        assert_same(res, want, len(widths))
        if low_bits is not None:
            assert res.stats()["order_overflow_runs"] > 0
        res.close()


def test_exactly_sized_rerun_after_a_low_prediction(oracle, jaspar579, monkeypatch):
    """A set far denser than the prediction: the predicted-size run is thrown away and the exactly-sized one orders the hits."""
    n = 80
    widths = jaspar579["widths"][:n]
    vals = jaspar579["pwm_values"][:4 * int(widths.sum())]
    cutoffs = jaspar579["cutoffs"]["1e-4"][:n]
    mats = synth.matrices_of(vals, widths)
    plain_b, plain_o = synth.make_regions(2000, 400, seed=71, frac_n=0.02, ragged=True)
    rng = np.random.default_rng(72)
    cons = ["".join("ACGT"[int(np.argmax(m[:, c]))] for c in range(m.shape[1])) for m in mats]
    dense = ["".join(cons[int(i)] for i in rng.integers(0, n, size=40)) for _ in range(1200)]
    draw, doff = _seqs(dense)
    want_plain = oracle.scan_arrays(vals, widths, cutoffs, plain_b.tobytes(), plain_o, 3, 8)
    want_dense = oracle.scan_arrays(vals, widths, cutoffs, draw, doff, 3, 8)
    for low_bits in (16, 24):
        _set_env(monkeypatch, low_bits=low_bits)
        pw = _lib.PwmSet(vals, widths, cutoffs)
        for _ in range(2):
            assert_same(_lib.scan(pw, _lib.SeqSet(plain_b, plain_o), 3), want_plain, n)
        res = _lib.scan(pw, _lib.SeqSet(draw, doff), 3)
        assert res.stats()["n_passes"] >= 2
        assert_same(res, want_dense, n)


def _edge_cases():
    rng = np.random.default_rng(9)
    words = ["".join(rng.choice(list("ACGT"), size=12)) for _ in range(6)]
    mats = [_word_motif(w) for w in words]
    cut = [0.97] * len(mats)
    bg = lambda n: "N" * n                                      # noqa: E731  (no window with an N scores)
    cases = {
        "no_hits": [bg(300), "ACGT" * 10, ""],
        "one_hit": [bg(50) + words[2] + bg(50)],
        "first_and_last_motif_only": [bg(40) + words[0] + bg(40) + words[5], bg(10), words[5] + "T" + words[0] * 3],
        "first_region_without_hits": [bg(500), bg(3), "".join(words) * 4, words[1]],
    }
    # regions at the rbits boundary (2^10 and 2^10 + 1 regions, the hits in the last ones), lengths at the pbits boundary
    for R in (1024, 1025):
        seqs = [bg(200)] * (R - 3) + [words[3] + bg(128 - 12), bg(256 - 12) + words[4], words[0] * 5]
        cases[f"R{R}"] = seqs
    cases["len_pow2"] = [bg(512 - 12) + words[1], words[2] + bg(512 - 24) + words[2], bg(511)]
    return _pack(mats, cut), cases


@pytest.mark.parametrize("strand", [1, 2, 3])
def test_edge_cases_at_every_low_bit_count(oracle, monkeypatch, strand):
    (vals, widths, cutoffs), cases = _edge_cases()
    P = len(widths)
    for name, seqs in cases.items():
        raw, offsets = _seqs(seqs)
        want = oracle.scan_arrays(vals, widths, cutoffs, raw, offsets, strand, 4)
        if name == "no_hits":
            assert len(want["pos"]) == 0
        if name == "one_hit" and strand == 1:
            assert len(want["pos"]) == 1
        if name == "first_and_last_motif_only" and len(want["pos"]):
            counts = np.diff(want["motif_offsets"])
            assert counts[1:-1].sum() == 0
        for low_bits, run_cap in ((None, None), (0, None), (8, None), (16, None), (24, None), (8, 1)):
            _set_env(monkeypatch, low_bits=low_bits, run_cap=run_cap)
            pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(raw, offsets)
            for _ in range(2):                                  # exactly sized, then predicted
                res = _lib.scan(pw, sq, strand)
                try:
                    assert_same(res, want, P)
                except AssertionError as e:
                    raise AssertionError(f"case {name}, low bits {low_bits}, cap {run_cap}: {e}") from None
                res.close()
