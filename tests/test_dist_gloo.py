"""
The N > 1 path on CPU: two processes, gloo backend, world_size 2.  The GPU scan itself cannot run
here, so the local scan function is injected (the oracle, test infrastructure); what is under test
is the host logic of motifscan_amd.dist: shard bounds balanced by bases, global region indices,
rank-order concatenation == single-process order, and the ONE all-reduce of the per-motif region
counts that feeds the enrichment statistics (stats.py:29-31).
"""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_scan(pwm_values, widths, cutoffs, bases, offsets, strand):
    from oracle import oracle
    r = oracle.scan_arrays(pwm_values, widths, cutoffs, bases.tobytes(), offsets, strand, 2)
    motif = np.repeat(np.arange(len(widths), dtype=np.int32), np.diff(r["motif_offsets"]))
    r["motif"] = motif
    pair = np.unique((motif.astype(np.int64) << 32) | r["seq_idx"])
    return r, np.bincount(pair >> 32, minlength=len(widths)).astype(np.int64)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from motifscan_amd import dist as msdist, synth
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        vals, widths, cutoffs = synth.load_motif_set(24)
        sets = [synth.make_regions(301, 300, seed=1, frac_n=0.05, ragged=True),
                synth.make_regions(257, 300, seed=2, frac_n=0.05, ragged=True)]
        out = msdist.scan_sharded(vals, widths, cutoffs, sets, rank, world, 3, scan_fn=oracle_scan)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), counts=out["counts"],
                 shards=np.array(out["shards"]),
                 **{f"s{s}_{k}": out["hits"][s][k] for s in range(2) for k in ("motif", "seq_idx", "pos", "score", "strand")})
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_shard_bounds_balance_and_cover():
    from motifscan_amd import dist as msdist
    rng = np.random.default_rng(0)
    lens = rng.integers(0, 2000, size=1000)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    for world in (1, 2, 3, 8):
        b = msdist.shard_bounds(offsets, world)
        assert b[0][0] == 0 and b[-1][1] == 1000
        assert all(b[k][1] == b[k + 1][0] for k in range(world - 1))
        sizes = [offsets[r1] - offsets[r0] for r0, r1 in b]
        assert max(sizes) - min(sizes) <= 2 * 2000
    # degenerate: fewer regions than ranks, empty set
    assert msdist.shard_bounds(np.array([0, 5]), 4)[-1][1] == 1
    assert msdist.shard_bounds(np.array([0]), 2) == [(0, 0), (0, 0)]


@pytest.mark.timeout(300)
def test_two_rank_gloo_scan_matches_single_process(tmp_path):
    import torch.multiprocessing as mp
    from motifscan_amd import synth
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r = [np.load(os.path.join(tmp_path, f"rank{k}.npz")) for k in range(world)]
    vals, widths, cutoffs = synth.load_motif_set(24)
    sets = [synth.make_regions(301, 300, seed=1, frac_n=0.05, ragged=True),
            synth.make_regions(257, 300, seed=2, frac_n=0.05, ragged=True)]
    assert np.array_equal(r[0]["counts"], r[1]["counts"])               # every rank holds the reduced counts
    for s, (bases, offsets) in enumerate(sets):
        whole, counts = oracle_scan(vals, widths, cutoffs, bases, offsets, 3)
        assert np.array_equal(r[0]["counts"][s], counts)
        assert r[0]["shards"][s][1] == r[1]["shards"][s][0]
        # rank-order concatenation, then a stable sort by motif, is the single-process order
        cat = {k: np.concatenate([r[0][f"s{s}_{k}"], r[1][f"s{s}_{k}"]]) for k in ("motif", "seq_idx", "pos", "score", "strand")}
        order = np.argsort(cat["motif"], kind="stable")
        for k in ("seq_idx", "pos", "score", "strand"):
            assert np.array_equal(cat[k][order], whole[k]), k
        assert len(whole["pos"]) > 50


def test_enrichment_consumes_reduced_counts():
    """fold change / Fisher p-values from the reduced counts == scipy on the same 2x2 tables
    (the reference's tests pin only counts and fold change: tests/test_stats.py:26-33)."""
    from scipy.stats import fisher_exact
    from motifscan_amd import dist as msdist
    rows = msdist.enrichment(np.array([30, 0, 5]), np.array([10, 0, 5]), 100, 200)
    assert rows[0][0] == 30 and rows[0][1] == 10 and rows[0][2] == pytest.approx(30 * 200 / 10 / 100)
    assert np.isnan(rows[1][2])
    assert rows[0][3] == fisher_exact([[30, 70], [10, 190]], alternative="greater")[1]
    assert rows[2][5] == min(min(rows[2][3], rows[2][4]) * 3, 1)


def test_sweep_shards_cover_every_window_once():
    from motifscan_amd import dist as msdist
    for begin, end, window, stride in ((0, 10_000, 200, 50), (17, 5003, 37, 10), (0, 150, 200, 50), (5, 1000, 64, 64)):
        n = (end - begin - window) // stride + 1 if end - begin >= window else 0
        for world in (1, 2, 3, 8):
            seen = []
            for rank in range(world):
                k0, k1, b, e = msdist.sweep_shard(begin, end, window, stride, rank, world)
                seen.extend(range(k0, k1))
                if k1 > k0:
                    assert b == begin + k0 * stride and e == begin + (k1 - 1) * stride + window and e <= end
                    assert (e - b - window) // stride + 1 == k1 - k0          # the span holds exactly the rank's windows
            assert seen == list(range(n))
    # the spans of a host-streamed genome sweep (bench.py --workload c5 --genome-mbp 240), shared by up to eight ranks: every rank
    # gets spans, and their window ranges tile the sweep in rank order
    from motifscan_amd import _lib, synth
    spans = _lib.sweep_spans(synth.c5_chrom_lengths(240_000_000), 200, 50, 375_000_000)
    n_windows = spans[-1][3] + spans[-1][4]
    for world in (1, 2, 4, 8):
        mine = [msdist.span_shard(spans, rank, world) for rank in range(world)]
        assert all(mine) and sum(mine, []) == spans
        ranges = [(m[0][3], m[-1][3] + m[-1][4]) for m in mine]
        assert ranges[0][0] == 0 and ranges[-1][1] == n_windows and all(x[1] == y[0] for x, y in zip(ranges[:-1], ranges[1:]))


def test_batch_bounds_cover_every_region_once_with_and_without_ramp():
    from motifscan_amd import dist as msdist
    for n in (0, 1, 5, 999, 1000, 1001, 4000, 125_000 * 8 + 17):
        for step in (1, 7, 250, 125_000):
            if n / step > 5000:
                continue
            for ramp in (False, True):
                for up, down in ((True, True), (True, False), (False, True), (False, False)):
                    b = msdist.batch_bounds(n, step, ramp=ramp, ramp_up=up, ramp_down=down)
                    assert b[0][0] == 0 and b[-1][1] == max(n, 0) or (n == 0 and b == [(0, 0)])
                    assert all(x[1] == y[0] for x, y in zip(b[:-1], b[1:])), (n, step, ramp)
                    assert all(0 < r1 - r0 <= (2 * step if ramp else step) for r0, r1 in b) or n == 0
    # a pass grows from a quarter of the batch size by doubling to twice it, and shrinks again at the end
    b = msdist.batch_bounds(1000, 100, ramp=True)
    assert [r1 - r0 for r0, r1 in b] == [25, 25, 50, 100, 200, 200, 200, 100, 50, 25, 25]
    b = msdist.batch_bounds(1_000_000, 125_000, max_batch=500_000, ramp_down=False)
    assert [r1 - r0 for r0, r1 in b] == [31_250, 31_250, 62_500, 125_000, 250_000, 500_000]
    b = msdist.batch_bounds(300, 100, ramp=True)                  # short sets keep round 2's cut of the first and last batch
    assert [r1 - r0 for r0, r1 in b] == [100, 100, 100]


def test_rank_shard_generation_fits_the_box(monkeypatch):
    """VERDICT r4 #7c: what every rank of an 8-GPU run does BEFORE it touches its GPU -- generate its own shard of both region sets
    in worker processes -- must not oversubscribe the host (8 ranks x their workers <= the box's cores) and must be quick: one
    rank's shard of the full configs[3] (125 000 regions of each set) well under 30 s on this container's 8 cores."""
    import time
    from motifscan_amd import synth
    for cores in (8, 64, 128, 256):
        monkeypatch.setattr(os, "cpu_count", lambda c=cores: c)
        for world in (1, 2, 4, 8):
            w = synth.default_workers(world)
            assert 1 <= w <= 16 and world * w <= max(cores, world)
    monkeypatch.undo()
    t0 = time.perf_counter()
    sh = synth.c4_shard(rank=5, world=8)
    dt = time.perf_counter() - t0
    assert dt < 30, dt
    assert sh["shard"] == (625_000, 750_000) and sh["n_regions"] == 125_000 and len(sh["sets"]) == 2
    assert all(len(b) == 125_000 * 500 and o[-1] == len(b) for b, o in sh["sets"])
    # rank 5's share is exactly block 5 of both sets: what the 1-GPU run scans at regions [625 000, 750 000)
    again = synth.make_regions(125_000, 500, seed=1000 * 5 + 1)[0]
    assert np.array_equal(sh["sets"][0][0], again)


# ---- the reference-side edits beyond the import swap, extracted and executed ----

def _cli_stub(tmp_dir):
    """The `motifscan/cli/scan_amd.py` block of INTEGRATION.md section 4, written out and imported."""
    import importlib.util
    import re
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    code = re.search(r"`motifscan/cli/scan_amd.py`:\s*```python\n(.*?)```", text, re.S).group(1)
    path = os.path.join(tmp_dir, "scan_amd_stub.py")
    if not os.path.exists(path):
        with open(path, "w") as fh:
            fh.write(code)
    spec = importlib.util.spec_from_file_location("scan_amd_stub", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Genome:
    def __init__(self, chroms):
        self._c = chroms
        self.chrom_sizes = {k: len(v) for k, v in chroms.items()}

    def fetch_sequence(self, chrom, start, end):
        return self._c[chrom][start:end]


class _Region:
    def __init__(self, chrom, start, end):
        self.chrom, self.start, self.end, self.summit = chrom, start, end, (start + end) // 2


class _Pwm:
    def __init__(self, i, m, cut):
        self.matrix, self.cutoffs, self.length = m, {"1e-4": cut}, m.shape[1]
        self.matrix_id, self.name = f"MA{i:04d}.1", f"motif{i}"


def cli_job(n_pwms=20):
    """A toy `motifscan scan` job: a 3-chromosome genome, 90 input regions, 130 control regions, windows of 200 bp, n_pwms motifs."""
    from motifscan_amd import synth
    vals, widths, cutoffs = synth.load_motif_set(n_pwms)
    mats = synth.matrices_of(vals, widths)
    bases, off = synth.make_regions(3, 6000, seed=9, frac_n=0.03)
    raw = bases.tobytes().decode()
    chroms = {f"chr{k + 1}": raw[int(off[k]):int(off[k + 1])] for k in range(3)}
    rng = np.random.default_rng(17)

    def regions(n):
        out = []
        for _ in range(n):
            c = f"chr{int(rng.integers(1, 4))}"
            a = int(rng.integers(0, 5600))
            out.append(_Region(c, a, a + int(rng.integers(50, 400))))
        return out
    return _Genome(chroms), [_Pwm(i, m, c) for i, (m, c) in enumerate(zip(mats, cutoffs))], regions(90), regions(130)


def expected_enrichment(pwms, sites_in, sites_ctl):
    """stats.py:18-45 as the reference runs it, on nested lists (the checker's own copy of the arithmetic; scipy's Fisher test)."""
    from scipy.stats import fisher_exact
    rows, n_motifs = [], len(sites_in)
    for pwm, a_l, c_l in zip(pwms, sites_in, sites_ctl):
        nt, ct = len(a_l), len(c_l)
        a, c = sum(len(x) > 0 for x in a_l), sum(len(x) > 0 for x in c_l)
        fold = a * ct / c / nt if nt > 0 and c > 0 else np.nan
        table = [[a, nt - a], [c, ct - c]]
        pe, pd_ = fisher_exact(table, "greater")[1], fisher_exact(table, "less")[1]
        rows.append((pwm.matrix_id + "," + pwm.name, a, c, fold, pe, pd_, min(min(pe, pd_) * n_motifs, 1)))
    return rows


def oracle_nested(pwms, scanner, strand=3):
    from oracle import oracle
    flat = oracle.c_scan_motif([p.matrix.tolist() for p in pwms], [p.cutoffs["1e-4"] for p in pwms], list(scanner.sequences), strand, 2)
    return oracle.make_motif_sites(flat, list(scanner.seq_starts))


def same_results(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert tuple(g)[:3] == w[:3]
        for x, y in zip(tuple(g)[3:], w[3:]):
            assert (np.isnan(x) and np.isnan(y)) or x == y


def _cli_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import pickle
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        stub = _cli_stub(out_dir if rank == 0 else os.path.join(out_dir, "r1"))
        genome, pwms, regions, control = cli_job()
        sites, results = stub.run_sharded(genome, pwms, regions, control, 200, "both", "1e-4", rank, world, scan_fn=oracle_scan)
        with open(os.path.join(out_dir, f"cli_rank{rank}.pkl"), "wb") as fh:
            pickle.dump({"sites": {k: np.asarray(v) for k, v in sites.items()}, "results": [tuple(r) for r in results]}, fh)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_integration_stub_of_the_sharded_cli_run(tmp_path):
    """the rank-sharded `run()` a maintainer would write, extracted from the document and run as two ranks
    over gloo (the local scan injected: the oracle).  Every rank ends with the enrichment results of the WHOLE job -- equal to
    stats.py:18-45 run on the nested lists of a single-process scan -- and the ranks' input sites, in rank order, are the
    single-process sites with global region indices and genome coordinates."""
    import pickle
    import torch.multiprocessing as mp
    from motifscan_amd.scanner import Scanner
    os.makedirs(tmp_path / "r1", exist_ok=True)
    world, port = 2, _free_port()
    mp.spawn(_cli_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r = [pickle.load(open(tmp_path / f"cli_rank{k}.pkl", "rb")) for k in range(world)]
    genome, pwms, regions, control = cli_job()
    sc_in, sc_ctl = Scanner(genome, regions, window_size=200), Scanner(genome, control, window_size=200)
    nested_in, nested_ctl = oracle_nested(pwms, sc_in), oracle_nested(pwms, sc_ctl)
    want = expected_enrichment(pwms, nested_in, nested_ctl)
    same_results(r[0]["results"], want)
    same_results(r[1]["results"], want)
    assert sum(w[1] for w in want) > 20 and sum(w[2] for w in want) > 20
    assert r[0]["sites"]["rows"][1] == r[1]["sites"]["rows"][0] and r[1]["sites"]["rows"][1] == len(regions)
    for m in range(len(pwms)):
        got = []
        for k in range(world):
            s = r[k]["sites"]
            a, b = int(s["motif_offsets"][m]), int(s["motif_offsets"][m + 1])
            got += list(zip(s["region"][a:b].tolist(), s["start"][a:b].tolist(), s["score"][a:b].tolist(), ["+" if x == 1 else "-" for x in s["strand"][a:b].tolist()]))
        flat = [(ri, st.start, st.score, st.strand) for ri, per in enumerate(nested_in[m]) for st in per]
        assert got == flat

