"""
The bucketed hit list (ms_fp64.hip's bucketed flush, ms_order.hip's bucket_plan_kernel / fill_tail_buckets_kernel, scan_bucket_decide in
ms_scan.hip): a predicted-size scan whose fp64 stage is rescore_carry_kernel writes its hits into 256 buckets of the radix digit
d0 = (key >> L) & 255, and the hit sort starts at bit L + 8.  The product takes that form for long lists only; here it is forced on short
ones.  Every case is compared, bit for bit, with the oracle AND with the same scans without buckets.

Measurement switches (honoured only with MS_MEASURE=1): MS_ORDER_BUCKETS=1 / 0 forces the form at any size / never, MS_ORDER_BUCKET_CAP caps
every bucket (the way to the overflow path), MS_SORT_LOW_BITS forces L, MS_RESCORE_SORTED_MIN=0 gives short candidate lists to
rescore_carry_kernel.  A PWM set's first scan has no prediction and is never bucketed: every case scans twice with one set.
"""
import numpy as np
import pytest

from motifscan_amd import _lib, synth

pytestmark = pytest.mark.gpu

N_MOTIFS = 50


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


def _set_env(monkeypatch, low_bits, buckets, cap=None):
    monkeypatch.setenv("MS_MEASURE", "1")
    monkeypatch.setenv("MS_RESCORE_SORTED_MIN", "0")
    for name, v in (("MS_SORT_LOW_BITS", low_bits), ("MS_ORDER_BUCKETS", buckets), ("MS_ORDER_BUCKET_CAP", cap)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _region_counts(want, P):
    off = want["motif_offsets"]
    return np.array([len(np.unique(want["seq_idx"][off[p]:off[p + 1]])) for p in range(P)], dtype=np.int64)


def _take(res):
    """everything a scan reports, copied: the five hit arrays, the per-motif offsets, the region counts, the statistics"""
    h = res.hits()
    out = {k: np.array(h[k]) for k in ("motif", "seq_idx", "pos", "strand", "score", "motif_offsets")}
    out["region_counts"] = np.asarray(res.region_counts(), dtype=np.int64).copy()
    out["stats"] = res.stats()
    res.close()
    return out


def _same(got, want, P, what):
    for k in ("motif_offsets", "seq_idx", "pos", "score"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs"
    assert np.array_equal(got["strand"].astype(np.int32), want["strand"].astype(np.int32)), f"{what}: strand differs"
    want_motif = np.repeat(np.arange(P, dtype=np.int32), np.diff(want["motif_offsets"]))
    assert np.array_equal(got["motif"], want_motif), f"{what}: motif differs"
    rc = want["region_counts"] if "region_counts" in want else _region_counts(want, P)
    assert np.array_equal(got["region_counts"], rc), f"{what}: region counts differ"


def _n_windows(offsets, widths):
    lens = np.diff(offsets)
    return sum(int(np.maximum(lens - int(w) + 1, 0).sum()) for w in widths)


def _expect_bucketed(motifs, offsets, want, low_bits, mu=None):
    """Whether the second scan of a set stays bucketed, from the host arithmetic (tests/test_bucket_plan_host.py) and the oracle's hits: the
    buckets are sized for a hit density that is uniform over (motif, window start) pairs, so motifs or regions far denser than the rest
    (a motif that hits ten times as often, a run of N under a weak motif) overflow theirs -- and the scan is run again, plain.
    True / False, None where a bucket is within one hit of its capacity (the library's mu is a rounded product), or "declined" where the
    gate refuses the layout even when forced (a digit that reaches into the motif bits, or a hit key that would tie with the padding keys).
    mu: the hits the library expects -- the previous scan's density times this set's windows; by default this set's own count (a re-scan)."""
    import math
    widths = np.asarray(motifs[1])
    P, R = len(widths), len(offsets) - 1
    bits = lambda n: max(1, int(n - 1).bit_length())                              # noqa: E731
    pbits, rbits, mbits = bits(int(np.diff(offsets).max())), bits(R), bits(P)
    gbits = rbits + pbits
    if gbits > int(offsets[-1]).bit_length() + 2:                # (region, position) keys would cost over two bits more than global positions: not used
        return "declined"
    motif = np.repeat(np.arange(P, dtype=np.int64), np.diff(want["motif_offsets"]))
    key = (motif << (gbits + 1)) | (want["seq_idx"].astype(np.int64) << (pbits + 1)) | (want["pos"].astype(np.int64) << 1)
    cnt = np.bincount(((key >> low_bits) & 255).astype(np.int64), minlength=256)
    mu = float(len(key)) if mu is None else float(mu)
    n_pred = int(mu * 1.06 + 6.0 * math.sqrt(mu + 1.0) + 256.0)                   # the first prediction's margin: 6 %
    kw = dict(offsets=offsets, widths=widths, gbits=gbits, pbits=pbits, end_bit=gbits + 1 + mbits, low_bits=low_bits, force=1)
    first = _lib.bucket_plan(mu, n_pred, **kw)
    if not first["gate"]:
        return "declined"
    n_pred = max(n_pred, first["need"])
    cap = _lib.bucket_plan(mu, n_pred, **kw)["cap"].astype(np.int64)
    if (cnt > cap + 1).any():
        return False
    return True if ((cnt < cap) | (cnt == 0)).all() else None


def _check_flags(runs, expect):
    """first scan: no prediction, plain; second: bucketed if no bucket overflows, else thrown away and run again, plain"""
    assert runs[0]["stats"]["order_bucketed"] == 0 and runs[0]["stats"]["n_passes"] == 1
    b, n = runs[1]["stats"]["order_bucketed"], runs[1]["stats"]["n_passes"]
    if expect == "declined":
        assert (b, n) == (0, 1)
        return
    assert (b, n) in ((1, 1), (0, 2))
    if expect is not None:
        assert b == (1 if expect else 0)


def _scans(monkeypatch, motifs, raw, offsets, strand, low_bits, buckets, n=2, cap=None, drop_cap_for_last=False):
    vals, widths, cutoffs = motifs
    _set_env(monkeypatch, low_bits, buckets, cap)
    pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(raw, offsets)
    out = []
    for i in range(n):
        if drop_cap_for_last and i == n - 1:
            _set_env(monkeypatch, low_bits, buckets, None)
        out.append(_take(_lib.scan(pw, sq, strand)))
    return out


def _mixed_regions():
    """2003 regions of 30 ... 200 bases (no multiple of 64), runs of one to four N in every ninth, lower case in every third; the regions
    whose index has low seven bits 40 ... 47, and the regions 1024 ... 1151, hold three bases -- shorter than any motif -- so
    that whole buckets stay empty at L = 8 (the digit: region bits 0 ... 6 and position bit 7).  19 coordinate bits: at L = 16 the digit
    would reach into the motif bits, and the gate declines."""
    rng = np.random.default_rng(2003)
    seqs = []
    for r in range(2003):
        n = int(rng.integers(30, 201))
        if 40 <= (r & 127) < 48 or (r >> 7) == 8:
            n = 3
        s = rng.choice(list("ACGT"), size=n, p=[.295, .205, .205, .295])
        if r % 9 == 0 and n > 20:
            for _ in range(2):
                st = int(rng.integers(0, n - 1))
                s[st:st + int(rng.integers(1, 5))] = "N"
        s = "".join(s)
        seqs.append(s.lower() if r % 3 == 2 else s)
    raw = "".join(seqs).encode()
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return raw, offsets


def _many_regions():
    """16 411 regions (15 region bits + 8 position bits: at L = 16 the digit is region bits 7 ... 14, coordinate bits only, as on the
    benchmark's default line; 1.2 Mbases, so that the keys carry (region, position)): 40 ... 100 bases, every sixteenth 30 ... 200; runs of N in every ninth, lower case in every third; regions
    1024 ... 1151 hold three bases.  129 of the 256 buckets can hold a hit."""
    rng = np.random.default_rng(16411)
    seqs = []
    for r in range(16411):
        n = int(rng.integers(30, 201)) if r % 16 == 5 else int(rng.integers(40, 101))
        if (r >> 7) == 8:
            n = 3
        s = rng.choice(list("ACGT"), size=n, p=[.295, .205, .205, .295])
        if r % 9 == 0 and n > 20:
            st = int(rng.integers(0, n - 1))
            s[st:st + int(rng.integers(1, 5))] = "N"
        s = "".join(s)
        seqs.append(s.lower() if r % 3 == 2 else s)
    raw = "".join(seqs).encode()
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return raw, offsets


@pytest.fixture(scope="module")
def many(oracle):
    motifs = synth.load_motif_set(N_MOTIFS, p_value="1e-3")
    raw, offsets = _many_regions()
    want = {s: oracle.scan_arrays(*motifs, raw, offsets, s, 8) for s in (1, 2, 3)}
    return motifs, raw, offsets, want


@pytest.fixture(scope="module")
def mixed(oracle):
    motifs = synth.load_motif_set(N_MOTIFS, p_value="1e-3")
    raw, offsets = _mixed_regions()
    want = {s: oracle.scan_arrays(*motifs, raw, offsets, s, 8) for s in (1, 2, 3)}
    return motifs, raw, offsets, want


@pytest.mark.parametrize("strand", [1, 2, 3])
@pytest.mark.parametrize("low_bits", [8, 16])
def test_mixed_regions_bucketed_equals_oracle_and_plain(mixed, monkeypatch, low_bits, strand):
    """The first scan of a set has no prediction and is plain, the second is bucketed; both equal the oracle and the unbucketed scans."""
    motifs, raw, offsets, want_all = mixed
    want = want_all[strand]
    assert len(want["pos"]) > (8000 if strand == 3 else 4000)      # enough for nearly every one of the 240 buckets that can hold a hit
    # the data leaves whole buckets empty: the digit of every hit key, key = motif << 20 | region << 9 | pos << 1 | strand bit
    motif = np.repeat(np.arange(N_MOTIFS, dtype=np.int64), np.diff(want["motif_offsets"]))
    key = (motif << 20) | (want["seq_idx"].astype(np.int64) << 9) | (want["pos"].astype(np.int64) << 1)
    assert 100 < len(np.unique((key >> low_bits) & 255)) < 256
    plain = _scans(monkeypatch, motifs, raw, offsets, strand, low_bits, 0)
    bucketed = _scans(monkeypatch, motifs, raw, offsets, strand, low_bits, 1)
    assert [r["stats"]["order_bucketed"] for r in plain] == [0, 0] and all(r["stats"]["n_passes"] == 1 for r in plain)
    expect = _expect_bucketed(motifs, offsets, want, low_bits)
    assert expect == (True if low_bits == 8 else "declined")     # L = 8: this set fits its buckets; L = 16: motif bits in the digit
    _check_flags(bucketed, expect)
    for i, (p, b) in enumerate(zip(plain, bucketed)):
        _same(b, want, N_MOTIFS, f"bucketed scan {i} against the oracle")
        _same(b, p, N_MOTIFS, f"bucketed scan {i} against the plain one")


@pytest.mark.parametrize("strand", [1, 2, 3])
def test_many_regions_bucketed_at_sixteen_low_bits(many, monkeypatch, strand):
    """L = 16 with a digit of region bits only -- the layout the product buckets: the second scan IS bucketed, its radix passes start at bit 24."""
    motifs, raw, offsets, want_all = many
    want = want_all[strand]
    assert len(want["pos"]) > (30000 if strand == 3 else 15000)
    motif = np.repeat(np.arange(N_MOTIFS, dtype=np.int64), np.diff(want["motif_offsets"]))
    key = (motif << 24) | (want["seq_idx"].astype(np.int64) << 9) | (want["pos"].astype(np.int64) << 1)
    assert 100 < len(np.unique((key >> 16) & 255)) <= 129
    plain = _scans(monkeypatch, motifs, raw, offsets, strand, 16, 0)
    bucketed = _scans(monkeypatch, motifs, raw, offsets, strand, 16, 1)
    assert [r["stats"]["order_bucketed"] for r in plain] == [0, 0] and all(r["stats"]["n_passes"] == 1 for r in plain)
    assert _expect_bucketed(motifs, offsets, want, 16) is True
    assert [(r["stats"]["order_bucketed"], r["stats"]["n_passes"]) for r in bucketed] == [(0, 1), (1, 1)]
    for i, (p, b) in enumerate(zip(plain, bucketed)):
        _same(b, want, N_MOTIFS, f"bucketed scan {i} against the oracle")
        _same(b, p, N_MOTIFS, f"bucketed scan {i} against the plain one")


def test_digit_that_reaches_into_the_motif_bits(oracle, monkeypatch):
    """Forty regions of at most 60 bases: 12 coordinate bits.  At L = 8 the digit would hold five coordinate and three motif bits, at
    L = 16 (cut to 13 by the layout) motif bits only: the gate declines both, forced or not, and the scans stay plain."""
    motifs = synth.load_motif_set(N_MOTIFS, p_value="1e-3")
    rng = np.random.default_rng(40)
    seqs = ["".join(rng.choice(list("ACGT"), size=int(n))) for n in rng.integers(20, 61, size=40)]
    raw = "".join(seqs).encode()
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    want = oracle.scan_arrays(*motifs, raw, offsets, 3, 4)
    assert len(want["pos"]) > 50
    for low_bits in (8, 16):
        plain = _scans(monkeypatch, motifs, raw, offsets, 3, low_bits, 0)
        bucketed = _scans(monkeypatch, motifs, raw, offsets, 3, low_bits, 1)
        e = _expect_bucketed(motifs, offsets, want, low_bits)
        assert e == "declined"
        _check_flags(bucketed, e)
        for p, b in zip(plain, bucketed):
            _same(b, want, N_MOTIFS, f"L = {low_bits} against the oracle")
            _same(b, p, N_MOTIFS, f"L = {low_bits} against the plain scan")


def test_bucket_overflow_reruns_once_and_switches_the_set_off(mixed, monkeypatch):
    """Buckets capped at four hits: the second scan overflows, its exactly-sized, plain re-run gives the result, and the set never
    buckets again -- the third scan, with the cap lifted, is plain and runs once."""
    motifs, raw, offsets, want_all = mixed
    runs = _scans(monkeypatch, motifs, raw, offsets, 3, 8, 1, n=3, cap=4, drop_cap_for_last=True)
    for i, r in enumerate(runs):
        _same(r, want_all[3], N_MOTIFS, f"scan {i}")
    assert [r["stats"]["order_bucketed"] for r in runs] == [0, 0, 0]
    assert [r["stats"]["n_passes"] for r in runs] == [1, 2, 1]
    assert all(r["stats"]["n_hits"] == len(want_all[3]["pos"]) for r in runs)


def test_counts_only_scan_is_never_bucketed(mixed, monkeypatch):
    motifs, raw, offsets, want_all = mixed
    want = want_all[3]
    got = {}
    for buckets in (0, 1):
        _set_env(monkeypatch, 8, buckets)
        pw, sq = _lib.PwmSet(*motifs), _lib.SeqSet(raw, offsets)
        got[buckets] = []
        for _ in range(2):
            res = _lib.scan(pw, sq, 3, _lib.MS_SCAN_COUNTS_ONLY)
            got[buckets].append((res.n_hits, np.array(res.motif_offsets), np.asarray(res.region_counts(), dtype=np.int64).copy(), res.stats()["order_bucketed"]))
            res.close()
    for a, b in zip(got[0], got[1]):
        assert a[0] == b[0] == len(want["pos"]) and a[3] == b[3] == 0
        assert np.array_equal(a[1], b[1]) and np.array_equal(b[1], want["motif_offsets"])
        assert np.array_equal(a[2], b[2]) and np.array_equal(b[2], _region_counts(want, N_MOTIFS))


def test_stream_of_two_batches(mixed, oracle, monkeypatch):
    """A batch stream: the first batch is sized exactly, the second from the first one's density -- queued, and bucketed when forced."""
    motifs, raw, offsets, _ = mixed
    cut = 1001
    b = np.frombuffer(raw, dtype=np.uint8)
    batches = [(b[:int(offsets[cut])], offsets[:cut + 1].copy()), (b[int(offsets[cut]):], offsets[cut:] - offsets[cut])]
    want = [oracle.scan_arrays(*motifs, bb.tobytes(), oo, 3, 8) for bb, oo in batches]
    got = {}
    for buckets in (0, 1):
        _set_env(monkeypatch, 8, buckets)
        pw = _lib.PwmSet(*motifs)
        got[buckets] = [_take(res) for res in _lib.scan_stream(pw, iter(batches), 3)]
    assert [r["stats"]["order_bucketed"] for r in got[0]] == [0, 0]
    # the library sizes batch 2 from batch 1's hits per window
    mu = len(want[0]["pos"]) / _n_windows(batches[0][1], motifs[1]) * _n_windows(batches[1][1], motifs[1])
    assert _expect_bucketed(motifs, batches[1][1], want[1], 8, mu) is True
    assert [(r["stats"]["order_bucketed"], r["stats"]["n_passes"]) for r in got[1]] == [(0, 1), (1, 1)]
    for i in range(2):
        _same(got[1][i], want[i], N_MOTIFS, f"batch {i} against the oracle")
        _same(got[1][i], got[0][i], N_MOTIFS, f"batch {i} against the plain stream")


def test_more_hits_than_the_stage_holds(oracle, monkeypatch):
    """Tandem ACGT under a palindromic word that hits on both strands at every fourth window, 4 Mbases of it so that the pre-filter's waves
    fill their candidate blocks: a round of 2048 candidates then makes up to 4096 hits, twice what a block stages, and the rest goes to the
    buckets one hit at a time."""
    word = "ACGTACGTACGT"
    m = np.full((4, len(word)), -3.0)
    for c, ch in enumerate(word):
        m["ACGT".index(ch), c] = 1.25
    vals, widths, cutoffs = synth.load_motif_set(3, p_value="1e-3")
    motifs = (np.concatenate([vals, m.ravel()]), np.concatenate([widths, [len(word)]]).astype(np.int32), np.concatenate([cutoffs, [0.95]]))
    rng = np.random.default_rng(12)
    seqs = ["ACGT" * int(k) for k in rng.integers(30, 51, size=20011)]
    raw = "".join(seqs).encode()
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    want = oracle.scan_arrays(*motifs, raw, offsets, 3, 8)
    assert len(want["pos"]) > 1_400_000
    plain = _scans(monkeypatch, motifs, raw, offsets, 3, 8, 0)
    bucketed = _scans(monkeypatch, motifs, raw, offsets, 3, 8, 1)
    expect = _expect_bucketed(motifs, offsets, want, 8)
    assert expect is True
    _check_flags(bucketed, expect)
    for p, b in zip(plain, bucketed):
        _same(b, want, 4, "against the oracle")
        _same(b, p, 4, "against the plain scan")
