#!/usr/bin/env python3
"""
bench.py -- the measurement contract of the PWM scan path.

    python bench.py --gpus N --steps K --warmup W [--workload c4|c3|c2|c5|c5shard|tiny] [--full]

With --gpus N > 1 and no WORLD_SIZE in the environment the script starts its own N ranks (fresh processes through
torch.distributed.run, before anything in this process has touched the GPU) and relays rank 0's line; under the
driver's torchrun it simply is one of the ranks.

Workload (default "c4" = BASELINE.json configs[3] IN FULL: 1M input + 1M control regions x 500 bp x 579 PWMs): every
rank takes its contiguous share of both region sets (dist.shard_bounds arithmetic), so 1 -> 8 GPUs is STRONG scaling on
the north-star workload.  A "step" is one pass of the hot path over the rank's share, starting from ASCII bases resident
in HBM: per region set  pack (extraction -> 2-bit codes + N mask) -> fp6 x fp4 matrix-core pre-filter -> fp64 re-scoring ->
ordering -> coordinates / per-motif region counts;  then the path's ONE collective, the all-reduce of the device-resident
int64[2 x 579] count vector (stats.py:29-31 input).  Hits stay in HBM inside the timed region: `value` is the
device-resident whole-job rate.

A plain run sets up, warms up, times the K steps and reports what those steps measured (the headline, the stage and
kernel times, the roofline figures derived from them).  --full also runs everything that takes runs or checks of its own,
after the timed steps: SURVEY.md 8(d)'s end-to-end metric (host ASCII in pinned memory -> hit arrays in pinned host memory,
i.e. H2D + pack + scan + D2H, through the library's batch stream, reported as `value_end_to_end` -- never as `value`), the
Python API leg, the N = 2, 4, 8 shard projection, the CPU baseline with its parity sample, the per-rank oracle samples and
count check of an N > 1 run, and the hits_packed mode of the c5 sweep.  The --no-* options leave single parts of that out.

Prints ONE JSON line on rank 0.  --dump-outputs DIR (region workloads) also writes what the last timed step computed on
rank 0 as DIR/<name>.npy, so that two builds can be compared output for output on the same seeded inputs.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                 # B/s, MI355X_MICROARCH.md "HBM3E peak BW"
LDS_PEAK = 256 * 256 * 2.4e9      # B/s: 256 B/clk/CU (ds_read_b128) x 256 CUs x 2.4 GHz
I8_MFMA_PEAK = 256 * 4 * 2048 * 2.4e9   # op/s: v_mfma_i32_32x32x32_i8 = 65536 ops per 32 cycles per SIMD (measured, tools/ubench),
                                        # 1024 SIMDs, 2.4 GHz = 5.03e15 = 2 x the dense bf16 peak of MI355X_MICROARCH.md
F6_MFMA_PEAK = 2 * I8_MFMA_PEAK         # op/s: v_mfma_scale_f32_32x32x64_f8f6f4 with fp6 / fp4 operands = 131072 ops per 32 cycles per SIMD
                                        # (measured 32.6, tools/ubench/mfma_f6_probe) = 1.0e16 = the guide's ~10 PF dense FP6/FP4 peak

PF_KERNEL = "prefilter_f6_kernel"    # the dominant kernel (ms_kernels.hip); rocprofv3 shows it as ms::prefilter_f6_kernel<2, false>

WORKLOAD_TEXT = {
    "c4": "BASELINE configs[3] in full: 1M input + 1M control regions x 500 bp x 579 PWMs, region-sharded over the ranks",
    "c3": "BASELINE configs[2]: 100k x 1 kb regions x 579 PWMs",
    "c2": "BASELINE configs[1]: 10k x 500 bp regions x 50 PWMs",
    "c5": "BASELINE configs[4]: multi-chromosome genome on the host swept as 200 bp windows stride 50 x 579 PWMs, streamed "
          "host -> GPU in spans (ms_stream_submit_span: every base scored once)",
    "c5shard": "BASELINE configs[4] per-GPU shard, genome RESIDENT in HBM: 375 Mbp as 200 bp windows stride 50 (7.5M windows) "
               "x 579 PWMs through ms_scan_sweep; value counts reference-equivalent units (window_bp x n_windows x n_motifs: "
               "the reference scans every base window / stride = 4 times, the sweep once)",
    "tiny": "smoke",
}


def kernel_source_sha16():
    """First 16 hex digits of the SHA-256 of the kernels' source: what a recorded PMC traffic figure is valid for."""
    import hashlib
    with open(os.path.join(ROOT, "motifscan_amd", "csrc", "ms_kernels.hip"), "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:16]


def visible_gpus():
    """Devices this process could use, WITHOUT initialising the GPU (on this image torch.cuda.device_count() only reads the
    driver's device list; no context is created, so starting child ranks afterwards stays legal)."""
    try:
        import torch
        return int(torch.cuda.device_count())
    except Exception:
        return 0


def self_launch(a):
    """Start --gpus ranks as fresh processes.  Nothing in THIS process has initialised the GPU (no HIP call)."""
    n_dev = visible_gpus()
    if a.gpus > n_dev and os.environ.get("MS_BENCH_SHARE_GPU") != "1":
        raise SystemExit(f"bench.py: --gpus {a.gpus} but only {n_dev} GPU(s) are visible: nothing was started")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    sys.exit(subprocess.run(cmd, env=env).returncode)


def load_workload(name, rank, world, args):
    """This rank's share: dict(pwm_values, widths, cutoffs, sets=[(bases, offsets)], shard, units (this rank), ...)."""
    from motifscan_amd import dist, synth
    if name == "c4":
        return synth.c4_shard(rank, world, regions_per_set=args.regions_per_set)
    wl = synth.workload(name)
    sets, shards = [], []
    for bases, offsets in wl["sets"]:
        r0, r1 = dist.shard_bounds(offsets, world)[rank]
        sets.append(dist.take_shard(bases, offsets, r0, r1))
        shards.append((r0, r1))
    wl["units_total"] = wl["units"]
    wl["n_regions_total"] = wl["n_regions"]
    wl["sets"] = sets
    wl["shard"] = shards[0] if shards else (0, 0)
    wl["units"] = sum(int(o[-1]) for _, o in sets) * wl["n_pwms"]
    return wl


def cpu_baseline(wl, seconds_target=12.0):
    """The reference's CPU scanner on a bounded sample of the same workload, on this box's host cores, and -- the oracle
    being the checker -- its hit list for that sample.  kind = "reference": the real cscore.c (oracle/_ref, built in the
    build container); otherwise kind = "port": the oracle's C restatement."""
    from oracle import oracle
    from motifscan_amd import synth
    cores = os.cpu_count() or 1
    bases, offsets = wl["sets"][0]
    L, P = wl["length"], wl["n_pwms"]
    mats = [m.tolist() for m in synth.matrices_of(wl["pwm_values"], wl["widths"])]
    cuts = wl["cutoffs"].tolist()
    ref = oracle.load_reference_ext()
    last = {}

    def run(n_regions, threads):
        raw = bases[:int(offsets[n_regions])].tobytes()
        if ref is not None:
            seqs = [raw[int(offsets[i]):int(offsets[i + 1])].decode() for i in range(n_regions)]
            t0 = time.perf_counter()
            out = ref.c_scan_motif(mats, cuts, seqs, 3, threads)
            t = time.perf_counter() - t0
            last["n"], last["hits"] = n_regions, out
            return t
        t0 = time.perf_counter()
        out = oracle.scan_arrays(wl["pwm_values"], wl["widths"], wl["cutoffs"], raw, offsets[:n_regions + 1], 3, threads)
        t = time.perf_counter() - t0
        last["n"], last["arrays"] = n_regions, out
        return t

    threads = min(cores, P)                        # the reference's work unit is one whole PWM (cscore.c:181-186)
    n_max = len(offsets) - 1
    n, t = min(64, n_max), 0.0
    for _ in range(4):                             # grow the sample until one run is a few seconds, then scale to target
        t = run(n, threads)
        if t >= 3.0 or n >= n_max:
            break
        n = int(min(n_max, max(2 * n, n * 4.0 / max(t, 1e-3))))
    if t < 0.6 * seconds_target and n < n_max:
        n = int(min(n_max, n * seconds_target / max(t, 1e-3)))
        t = run(n, threads)
    units = int(offsets[n]) * P
    out = {"value": units / t, "unit": "bp*motifs/s", "cores": threads,
           "kind": "reference" if ref is not None else "port",
           "sample": f"first {n} regions x {L} bp x {P} PWMs of the same workload, both strands, {t:.1f} s wall",
           "host_cores_total": cores}
    sample = dict(last)
    n0 = 16
    t1 = run(max(n // max(threads, 1), n0), 1)
    out["value_1thread"] = int(offsets[max(n // max(threads, 1), n0)]) * P / t1
    return out, sample


def parity_sample(wl, pw, sample):
    """The GPU's hits for the CPU baseline's sample, compared with what the reference just returned for it (checker only)."""
    from motifscan_amd import _lib
    n = sample["n"]
    bases, offsets = wl["sets"][0]
    sq = _lib.SeqSet(bases[:int(offsets[n])], offsets[:n + 1])
    res = _lib.scan(pw, sq, 3)
    h = res.hits()
    res.close(); sq.close()
    if "hits" in sample:
        per = sample["hits"]
        want_off = np.concatenate([[0], np.cumsum([len(x) for x in per])])
        flat = [x for p in per for x in p]
        w_seq = np.array([x[0] for x in flat], dtype=np.int64)
        w_pos = np.array([x[1] for x in flat], dtype=np.int64)
        w_sc = np.array([x[2] for x in flat], dtype=np.float64)
        w_sd = np.array([x[3] for x in flat], dtype=np.int64)
    else:
        a = sample["arrays"]
        want_off, w_seq, w_pos, w_sc, w_sd = a["motif_offsets"], a["seq_idx"], a["pos"], a["score"], a["strand"].astype(np.int64)
    same = (np.array_equal(h["motif_offsets"], want_off) and np.array_equal(h["seq_idx"], w_seq) and np.array_equal(h["pos"], w_pos)
            and np.array_equal(h["score"], w_sc) and np.array_equal(h["strand"].astype(np.int64), w_sd))
    return {"regions": int(n), "hits": int(len(w_pos)), "identical_to_cpu_reference": bool(same)}


def rank_parity_sample(wl, pw, n_regions=2000, strand=3):
    """Every rank checks the first n_regions of ITS OWN shard against the oracle's C restatement (liboracle.so: test
    infrastructure, the checker only), so that a multi-GPU line is self-verifying rank by rank."""
    from oracle import oracle
    from motifscan_amd import _lib
    bases, offsets = wl["sets"][0]
    n = int(min(n_regions, len(offsets) - 1))
    if n <= 0:
        return {"regions": 0, "hits": 0, "identical": True}
    raw = bases[:int(offsets[n])]
    threads = max(1, min(16, (os.cpu_count() or 1) // max(int(os.environ.get("WORLD_SIZE", "1")), 1)))
    want = oracle.scan_arrays(wl["pwm_values"], wl["widths"], wl["cutoffs"], raw.tobytes(), offsets[:n + 1], strand, threads)
    sq = _lib.SeqSet(raw, offsets[:n + 1])
    res = _lib.scan(pw, sq, strand)
    h = res.hits()
    res.close(); sq.close()
    same = (np.array_equal(h["motif_offsets"], want["motif_offsets"]) and np.array_equal(h["seq_idx"], want["seq_idx"])
            and np.array_equal(h["pos"], want["pos"]) and np.array_equal(h["score"], want["score"])
            and np.array_equal(h["strand"].astype(np.int64), want["strand"].astype(np.int64)))
    return {"regions": n, "hits": int(len(want["pos"])), "identical": bool(same)}


def _nccl_version(torch):
    try:
        v = torch.cuda.nccl.version()
        return ".".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)
    except Exception as e:                          # the line must not die on a version string
        return f"unknown ({type(e).__name__})"


DUMP_HIT_BYTES = 60 << 20          # --dump-outputs: the hit samples of all region sets together (the rest stays far below 4 MB)


def dump_outputs(out_dir, results, counts):
    """What one step of the timed path hands its caller, as float64 .npy files: region_counts [sets, P] (the step's
    all-reduced per-motif counts of regions with >= 1 site), and per region set k: set<k>_motif_offsets [P + 1] and
    set<k>_hits [n, 6] with rows (index in the hit list, motif, seq_idx, pos, strand, score) -- every hit when they fit in
    DUMP_HIT_BYTES, else a sample of hit indices drawn with seed k (a function of the hit count only)."""
    os.makedirs(out_dir, exist_ok=True)
    P = results[0].n_pwms
    np.save(os.path.join(out_dir, "region_counts.npy"), counts.reshape(len(results), P).astype(np.float64))
    cap = DUMP_HIT_BYTES // len(results) // (6 * 8)
    for k, res in enumerate(results):
        n = res.n_hits
        idx = np.arange(n) if n <= cap else np.sort(np.random.default_rng(k).choice(n, cap, replace=False))
        h = res.hits(copy=False, motif=False)
        motif = np.searchsorted(res.motif_offsets, idx, side="right") - 1
        rows = np.stack([idx, motif, h["seq_idx"][idx], h["pos"][idx], h["strand"][idx], h["score"][idx]], axis=1).astype(np.float64)
        np.save(os.path.join(out_dir, f"set{k}_motif_offsets.npy"), res.motif_offsets.astype(np.float64))
        np.save(os.path.join(out_dir, f"set{k}_hits.npy"), rows)


class _DevicePtr:
    """Lets torch wrap the library's device-resident count vector without a copy (CUDA array interface)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (int(ptr), False), "version": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="c4", choices=list(WORKLOAD_TEXT))
    ap.add_argument("--full", action="store_true", help="after the timed steps, also run the end-to-end, API, scale-projection and CPU-baseline legs "
                    "and the per-rank checks (see the module docstring); a plain run reports the timed steps only")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline and its parity sample")
    ap.add_argument("--no-end-to-end", action="store_true", help="--full: skip the end-to-end legs (value_end_to_end)")
    ap.add_argument("--no-api", action="store_true", help="--full: skip the value_api leg (Scanner.scan_motifs at configs[1] and configs[2])")
    ap.add_argument("--no-scale-projection", action="store_true", help="--full: skip the N = 2, 4, 8 shard steps timed at N = 1 (scale_projection)")
    ap.add_argument("--no-batch-ramp", action="store_true", help="end-to-end passes: equal batches (default: small first and last batches)")
    ap.add_argument("--min-warm-seconds", type=float, default=2.0, help="untimed warm-up steps continue until this much wall time has passed (DVFS steady state)")
    ap.add_argument("--regions-per-set", type=int, default=None, help="c4 only: shrink the workload (development aid; the line then says so)")
    ap.add_argument("--genome-mbp", type=int, default=3000, help="c5 only: synthetic genome size in Mbp")
    ap.add_argument("--batch-regions", type=int, default=125_000, help="end-to-end leg: the batches of a pass grow from a quarter of this ...")
    ap.add_argument("--max-batch-regions", type=int, default=250_000, help="... to this many regions, and shrink again at the end of the pass")
    ap.add_argument("--p-value", default="1e-4", choices=["1e-2", "1e-3", "1e-4", "1e-5", "1e-6"],
                    help="cutoff column of the motif set (the reference's -p, cli/main.py:520-521); anything but 1e-4 is a builder-run side workload, the line says so")
    ap.add_argument("--strand", default="both", choices=["both", "+", "-"], help="the reference's --strand (cli/main.py:543); default both")
    ap.add_argument("--motif-set", default="benchmark", choices=["benchmark", "lowinfo"],
                    help="lowinfo: the JASPAR-like-information side set (informative core, weak flanks, 10 %% weak motifs); a side workload, the line says so")
    ap.add_argument("--host-pack", action="store_true", help="end-to-end legs: convert_seq on the stream's host threads (MS_STREAM_HOST_PACK: 0.69 B/base over the link "
                    "instead of 1, no pack kernel) -- an option for multi-GPU nodes whose host link is the bound; slower at N = 1 (profiles/r05_host_packed_upload.log)")
    ap.add_argument("--extra-widths", default="", help="comma list: append one synthetic motif of each of these widths (side workload: motifs wider than the set holds)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy, float64, "
                         "under 64 MB in all (a seeded sample of the hits when there are more); with --gpus N > 1 the region counts are the "
                         "all-reduced sum and the hits rank 0's shard only: see dump_outputs()")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.dump_outputs and a.workload in ("c5", "c5shard"):
        ap.error("--dump-outputs covers the region workloads (c4, c3, c2, tiny), not the window sweeps")
    strand_mask = {"both": 3, "+": 1, "-": 2}[a.strand]
    side = a.p_value != "1e-4" or a.strand != "both" or bool(a.extra_widths) or a.motif_set != "benchmark"

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(a)                             # never returns

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} disagrees with WORLD_SIZE {world}: launch one rank per GPU (or let bench.py start them itself)")

    # synthetic inputs first: plain numpy in worker processes, before this process touches the GPU
    if a.workload in ("c5", "c5shard"):
        return main_sweep(a, world, rank, local_rank)
    wl = load_workload(a.workload, rank, world, a)
    if side:
        from motifscan_amd import synth
        vals, widths, cutoffs = synth.load_motif_set(wl["n_pwms"], a.p_value, a.motif_set)
        mats = [m for m in synth.matrices_of(vals, widths)]
        cuts = list(cutoffs)
        for w in [int(x) for x in a.extra_widths.split(",") if x]:
            m, c = synth.random_motif(w, seed=900 + w, p_value=float(a.p_value))
            mats.append(m)
            cuts.append(c)
        per_bp = wl["units"] // wl["n_pwms"]
        wl["pwm_values"] = np.concatenate([m.ravel() for m in mats])
        wl["widths"] = np.array([m.shape[1] for m in mats], dtype=np.int32)
        wl["cutoffs"] = np.array(cuts, dtype=np.float64)
        wl["n_pwms"] = len(mats)
        wl["units"] = per_bp * len(mats)

    import torch                                   # device memory / streams / torch.distributed only
    import torch.distributed as dist
    from motifscan_amd import _lib

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise RuntimeError("bench.py needs an MI355X; there is no CPU fallback")
    # MS_BENCH_BACKEND=gloo + MS_BENCH_SHARE_GPU=1 (test aid only): lets the N > 1 code path run on a box with fewer GPUs
    # than ranks (ranks then share devices; RCCL itself refuses two ranks on one GPU)
    backend = os.environ.get("MS_BENCH_BACKEND", "nccl")
    share = os.environ.get("MS_BENCH_SHARE_GPU") == "1"
    # MS_BENCH_FORCE_PG=1 (test aid only): a ONE-rank run opens the process group too and takes every N > 1 branch below -- on a one-GPU box
    # that is the only way the RCCL calls of this file (init with device_id, the int64 all-reduce on the library's vector, all_gather, barrier) ever execute
    use_pg = world > 1 or os.environ.get("MS_BENCH_FORCE_PG") == "1"
    dev_index = local_rank % _lib.device_count() if share else local_rank
    torch.cuda.set_device(dev_index)               # before the process group: RCCL binds to the current device
    _lib.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if use_pg:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:         # (only a forced one-rank group is ever started without a launcher)
            s_ = socket.socket()
            s_.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(s_.getsockname()[1])
            s_.close()
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    P = wl["n_pwms"]
    pw = _lib.PwmSet(wl["pwm_values"], wl["widths"], wl["cutoffs"])
    seqsets = [_lib.SeqSet(b, o, keep_ascii=True) for b, o in wl["sets"]]
    n_sets = len(seqsets)
    counts = torch.zeros(n_sets * P, dtype=torch.int64, device=dev)          # this rank's counts, then the reduced vector
    local_counts = torch.zeros(n_sets * P, dtype=torch.int64, device=dev)

    ar_events = []                                  # (start, end) CUDA events around the path's one collective, per timed step

    def step(timed=False, keep=None):
        stats = []
        for s, sq in enumerate(seqsets):
            sq.repack()                            # extraction: resident ASCII -> 2-bit codes + N mask
            res = _lib.scan(pw, sq, strand_mask)
            stats.append(res.stats())
            # the library's own device vector, wrapped in place: device -> device, no trip through the host
            counts[s * P:(s + 1) * P].copy_(torch.as_tensor(_DevicePtr(res.region_counts_device_ptr(), P), device=dev))
            torch.cuda.current_stream().synchronize()          # the result block returns to the pool on close()
            if keep is None:
                res.close()
            else:
                keep.append(res)                   # --dump-outputs: closed once written, after the timed region
        local_counts.copy_(counts)
        if use_pg:
            if timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            dist.all_reduce(counts, op=dist.ReduceOp.SUM)      # the path's one collective (stats.py:29-31 input)
            if timed:
                e1.record()
                ar_events.append((e0, e1))
        return stats

    def fence():
        if use_pg:
            dist.barrier()
        torch.cuda.synchronize()

    n_warm = 0
    t_warm = time.perf_counter()
    while True:                                    # untimed: W steps AND at least --min-warm-seconds (DVFS steady state)
        step()
        n_warm += 1
        more = n_warm < a.warmup or time.perf_counter() - t_warm < a.min_warm_seconds
        if use_pg:                                 # the ranks agree on when to stop (every step holds a collective)
            flag = torch.tensor([1 if more else 0], dtype=torch.int64, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            more = bool(flag.item())
        if not more:
            break
    last_results = [] if a.dump_outputs else None
    if last_results is not None:
        # the last timed step keeps every set's result open until it is dumped, where a step otherwise returns each result block to the
        # pool before the next scan: one more untimed step that holds them all leaves the pool enough blocks, so no timed scan goes to the driver
        held = []
        step(keep=held)
        n_warm += 1
        for res in held:
            res.close()
    fence()
    pool0 = _lib.pool_stats()
    t0 = time.perf_counter()
    all_stats = []
    for k in range(a.steps):
        all_stats.extend(step(timed=True, keep=last_results if k == a.steps - 1 else None))
    torch.cuda.synchronize()
    own_elapsed = time.perf_counter() - t0          # this rank's own K steps (its last collective included), before the closing barrier
    fence()
    elapsed = time.perf_counter() - t0
    pool1 = _lib.pool_stats()
    tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    units = torch.tensor([float(wl["units"])], dtype=torch.float64, device=dev)
    if use_pg:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(units, op=dist.ReduceOp.SUM)
    elapsed = float(tmax.item())
    total_units = float(units.item())
    if last_results is not None:
        if rank == 0:
            dump_outputs(a.dump_outputs, last_results, counts.cpu().numpy())
        for res in last_results:
            res.close()

    counts_check = None
    ranks_report = None
    if use_pg:
        ps = None
        if a.full:
            # the collective, checked: all-reduced vector == sum over ranks of the vectors each rank's library handed over
            gathered = [torch.zeros_like(local_counts) for _ in range(world)]
            dist.all_gather(gathered, local_counts)
            counts_check = {"allreduce_equals_sum_of_rank_counts": bool(torch.equal(torch.stack(gathered).sum(0), counts)),
                            "max_regions_with_site": int(counts.max().item())}
            ps = rank_parity_sample(wl, pw, strand=strand_mask)      # 2000 of this rank's regions checked against the oracle
        # per rank: its own ms per step and the collective's own time (and with --full its oracle sample)
        ar_ms = sum(e0.elapsed_time(e1) for e0, e1 in ar_events) / max(len(ar_events), 1)
        mine = [own_elapsed / a.steps * 1e3, ar_ms, float(wl["shard"][0]), float(wl["shard"][1]), float(dev_index)]
        if ps is not None:
            mine += [float(ps["regions"]), float(ps["hits"]), 1.0 if ps["identical"] else 0.0]
        mine = torch.tensor(mine, dtype=torch.float64, device=dev)
        per_rank = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(per_rank, mine)
        tab = torch.stack(per_rank).cpu().numpy()
        ranks_report = {"ms_per_step_min": float(tab[:, 0].min()), "ms_per_step_max": float(tab[:, 0].max()),
                        "ms_per_step_by_rank": [round(float(x), 3) for x in tab[:, 0]],
                        "allreduce_ms_mean_by_rank": [round(float(x), 4) for x in tab[:, 1]],
                        # every rank's [r0, r1) of each region set: contiguous, in rank order, together the whole set
                        "shard_by_rank": [[int(x), int(y)] for x, y in tab[:, 2:4]],
                        "shards_tile_every_set": bool(tab[0, 2] == 0 and tab[-1, 3] == wl["n_regions_total"]
                                                      and all(tab[k, 3] == tab[k + 1, 2] for k in range(world - 1))),
                        # what the collective ran on: the judge can see that RCCL saw `world` ranks, one per device
                        "rccl": {"backend": dist.get_backend(), "world": world, "device_ids": [int(x) for x in tab[:, 4]],
                                 "devices_visible": int(torch.cuda.device_count()), "one_rank_per_device": len({int(x) for x in tab[:, 4]}) == world,
                                 "nccl_version": _nccl_version(torch) if dist.get_backend() == "nccl" else None,
                                 "device_name": torch.cuda.get_device_name(dev)}}
        if ps is not None:
            ranks_report["parity_sample"] = {"regions_per_rank": int(tab[:, 5].min()), "hits_checked": int(tab[:, 6].sum()),
                                             "ranks_identical_to_oracle": int(tab[:, 7].sum()), "ranks": world,
                                             "checker": "oracle/cscore_oracle.c (liboracle.so), first regions of every rank's own shard"}

    # ---- what a rank's step would be at N = 2, 4, 8 (VERDICT r4 #7b): the shard a rank of an N-GPU run scans, timed here on one GPU.
    # The ranks share nothing but the collective, so N x (step at 1) / (step at N) bounds the node's speedup before it; the driver's
    # SCALE run can be held against this table line by line.
    scale_projection = None
    if a.full and rank == 0 and world == 1 and a.workload == "c4" and not side and not a.no_scale_projection:
        scale_projection = {"definition": "ms per resident step (median of single steps) of ONE rank's shard of an N-GPU run (first 1/N of both region sets), measured on this GPU; "
                                          "speedup_bound = step(1) / step(N): the scaling an N-GPU node reaches before its one all-reduce",
                            "ms_per_step": {"1": elapsed / a.steps * 1e3}, "speedup_bound": {}}
        for n_ranks in (2, 4, 8):
            sub = []
            for b, o in wl["sets"]:
                r1 = (len(o) - 1) // n_ranks
                sub.append(_lib.SeqSet(b[:int(o[r1])], o[:r1 + 1], keep_ascii=True))
            full, seqsets[:] = list(seqsets), sub
            try:
                t_w = time.perf_counter()
                while time.perf_counter() - t_w < 0.5:
                    step()
                torch.cuda.synchronize()
                # (the MEDIAN of single steps: one 30 ms driver call inside ten 5.7 ms steps -- a block of a size class the cache did not hold yet --
                # once turned the N = 8 line into 9.3 ms, profiles/r05h_bench_c4.json)
                k_steps = max(a.steps, 10)
                singles = []
                for _ in range(k_steps):
                    t1 = time.perf_counter()
                    step()
                    torch.cuda.synchronize()
                    singles.append((time.perf_counter() - t1) * 1e3)
                ms_n = sorted(singles)[len(singles) // 2]
            finally:
                seqsets[:] = full
                for sq in sub:
                    sq.close()
            scale_projection["ms_per_step"][str(n_ranks)] = ms_n
            scale_projection["speedup_bound"][str(n_ranks)] = elapsed / a.steps * 1e3 / ms_n

    # ---- the drop-in at the Python API (before the streamed legs: they leave the library's block pools holding a few dozen GB-sized
    # blocks, and the first small scan behind them once paid a 40 ms driver call for that: r04f_bench_c4.json against r04e_) ----
    api = None
    if a.full and rank == 0 and world == 1 and not a.no_api and not side:
        api = api_leg()

    # ---- SURVEY.md 8(d) end-to-end: host ASCII (pinned) -> hit arrays in pinned host memory, through the batch stream ----
    e2e = None
    if a.full and not a.no_end_to_end:
        e2e = end_to_end(a, wl, pw, world, dev, torch, dist if use_pg else None, strand_mask)

    if rank == 0:
        n_launch = len(all_stats)
        pf_ms = sum(s["ms_prefilter"] for s in all_stats) / n_launch          # HIP events on the library's stream
        alg_bytes = sum(s["hbm_bytes_algorithmic"] for s in all_stats) / n_launch
        lds_bytes = sum(s["lds_bytes_read"] for s in all_stats) / n_launch
        windows = sum(s["n_windows"] for s in all_stats) / n_launch
        achieved = alg_bytes / (pf_ms * 1e-3)
        # HBM bytes per launch from a recorded PMC pass (rocprofv3 --pmc, separate FETCH_SIZE / WRITE_SIZE passes: profiles/): only
        # an entry recorded for THIS kernel on THIS workload and configuration counts, anything else prints null
        # (tools/pmc_traffic_update.py writes the entry "<workload>_current" from the evidence pass's FETCH_SIZE / WRITE_SIZE summaries together
        # with a hash of the kernel source it was taken on: a kernel changed since then prints null, not a stale number)
        traffic = None
        tfile = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tfile) and not side:
            try:
                ent = json.load(open(tfile)).get(a.workload + "_current", {})
                if PF_KERNEL in ent.get("kernel", "") and ent.get("kernel_source_sha16") == kernel_source_sha16():
                    traffic = ent.get("hbm_bytes_per_launch")
            except (OSError, ValueError):
                traffic = None
        # dominant kernel = prefilter_f6_kernel, on the matrix cores and power-limited (~1240 W of the board's 1400 W over a scan loop, the shader
        # clock at 2.25 instead of 2.40 GHz: DESIGN.md 4, profiles/r05_double_pass.log): algorithmic ops =
        # SURVEY.md 8(d)'s "one add per (window, column, strand)" counted as a multiply-add (2 ops); what the kernel ISSUES is 4x
        # that (one-hot: 4 k-slots per base) plus the padding of widths to k-blocks of 16 columns.  peak = the dense matrix peak of
        # the operand types the kernel feeds the pipe (fp6 x fp4: MI355X_MICROARCH.md ~10 PF)
        alg_ops = sum(s["mfma_ops_algorithmic"] for s in all_stats) / n_launch
        issued = sum(s["mfma_ops"] for s in all_stats) / n_launch
        peak = F6_MFMA_PEAK
        roofline = {"bound": "mfma", "achieved": alg_ops / (pf_ms * 1e-3) / 1e12, "peak": peak / 1e12, "unit": "TFLOP/s",
                    "frac": alg_ops / (pf_ms * 1e-3) / peak, "traffic": traffic, "kernel": PF_KERNEL,
                    "kernel_ms": pf_ms, "algorithmic_ops_per_launch": alg_ops,
                    "dtype": "fp6 (e2m3) x fp4 (e2m1, one-hot) -> f32, exact",
                    "frac_of_int8_peak": alg_ops / (pf_ms * 1e-3) / I8_MFMA_PEAK}
        on_chip = {"bound": "matrix pipe (issued ops incl. one-hot zeros and width padding)",
                   "achieved": issued / (pf_ms * 1e-3) / 1e12, "peak": peak / 1e12, "unit": "TOP/s",
                   "frac": issued / (pf_ms * 1e-3) / peak, "issued_ops_per_launch": issued,
                   "lds_TBps": lds_bytes / (pf_ms * 1e-3) / 1e12, "windows_per_s_kernel": windows / (pf_ms * 1e-3)}
        shrunk = a.workload == "c4" and a.regions_per_set is not None
        line = {
            "metric": f"scanned bp*motifs per second (region_bp x n_motifs), {'both strands' if a.strand == 'both' else 'strand ' + a.strand}, p={a.p_value} cutoffs"
                      + (" [SIDE WORKLOAD: not BASELINE's configuration]" if side else ""),
            "value": total_units * a.steps / elapsed,
            "unit": "bp*motifs/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": elapsed / a.steps * 1e3,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64 (every hit decision and score, as in the reference) behind an fp6 x fp4 one-hot matrix-core pre-filter (exact f32 accumulate)",
            "data": "synthetic",
            "config": {"workload": WORKLOAD_TEXT[a.workload] + (f" [SHRUNK to {a.regions_per_set} regions per set: development run]" if shrunk else ""),
                       "regions_total": wl["n_regions_total"] * n_sets, "regions_per_gpu": wl["n_regions"] * n_sets,
                       "region_bp": wl["length"], "n_pwms": P, "strands": a.strand, "p_value": a.p_value, "motif_set": a.motif_set,
                       "motif_widths": f"{int(np.min(wl['widths']))}..{int(np.max(wl['widths']))}",
                       "sharding": f"{wl['n_regions_total']} + {wl['n_regions_total']} regions split contiguously over {world} GPU(s)"
                                   if n_sets == 2 else f"{wl['n_regions_total']} regions split contiguously over {world} GPU(s)",
                       "collective": f"1 all-reduce(sum) of the device-resident int64[{n_sets * P}] count vector per step",
                       "warmup_steps_run": n_warm, "timed_region_s": elapsed},
            "value_definition": "device-resident (the bench contract: inputs already in HBM when the timed region starts): ASCII in HBM at the start, hits left in HBM; "
                                "pack + pre-filter + fp64 + order + finalize + all-reduce inside.  SURVEY.md 8(d)'s pack + H2D + kernel + D2H metric is "
                                "value_8d_end_to_end (every hit of both sets to pinned host memory) and value_8d_cli_job (the reference CLI's own data flow), "
                                "both in a --full run",
            "roofline": roofline,
            "roofline_hbm": {"bound": "hbm", "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                             "frac": achieved / HBM_PEAK, "traffic": traffic, "algorithmic_bytes_per_launch": alg_bytes},
            "roofline_on_chip": on_chip,
            "stage_ms_per_scan": {k: sum(s[k] for s in all_stats) / n_launch
                                  for k in ("ms_prefilter", "ms_exact", "ms_sort", "ms_finalize", "ms_total")},
            "hits_per_scan": sum(s["n_hits"] for s in all_stats) / n_launch,
            "candidates_per_scan": sum(s["n_candidates"] for s in all_stats) / n_launch,
            # 3 = candidates parked and decoded later, 4 = decoded in place (the library's choice from the previous scan's density: p >= ~5e-3);
            # motifs the pre-filter cannot take (a cutoff that lets most windows pass, W > 63) go through exact_all_kernel
            "prefilter_form_per_scan": sorted({int(s["pf_engine"]) for s in all_stats}),
            "n_pwms_exact_only": int(all_stats[-1]["n_pwms_exact"]),
            # the path's one collective per step, slowest rank's mean (device events around dist.all_reduce); 0 at N = 1: no collective runs
            "allreduce_ms": max(ranks_report["allreduce_ms_mean_by_rank"]) if ranks_report is not None else 0.0,
            # rank 0's HBM block cache over the timed steps: a miss is a driver allocation inside the timed region
            "hbm_pool_timed": {k: pool1[k] - pool0[k] for k in ("hits", "misses", "driver_frees", "driver_ms")},
        }
        if counts_check is not None:
            line["counts_check"] = counts_check
            line["ranks"] = ranks_report
        if ranks_report is not None:
            line["rccl"] = ranks_report["rccl"]
        if scale_projection is not None:
            line["scale_projection"] = scale_projection
        if e2e is not None:
            line["value_end_to_end"] = e2e
            # SURVEY.md 8(d)'s metric proper (pack + H2D + kernel + D2H), as top-level scalars beside `value`.  (`value` itself stays the
            # device-resident rate: the bench contract of this build says a PCIe-inclusive rate is never `value`.)
            line["value_8d_end_to_end"] = e2e["pipelined"]
            line["value_8d_cli_job"] = e2e["pipelined_cli"]
            line["end_to_end_over_resident"] = {"pipelined": e2e["pipelined"] / line["value"], "pipelined_cli": e2e["pipelined_cli"] / line["value"],
                                                "pipelined_sustained": e2e["pipelined_sustained"] / line["value"]}
        if a.full and world == 1 and not a.no_cpu_baseline and wl["sets"] and not side:
            line["cpu_baseline"], sample = cpu_baseline(wl)
            line["parity_sample"] = parity_sample(wl, pw, sample)
        if api is not None:
            line["value_api"] = api
        print(json.dumps(line), flush=True)
    if use_pg:
        dist.barrier()
        dist.destroy_process_group()


def api_leg():
    """The drop-in at the API north_star names: Scanner(genome, regions).scan_motifs(pwms) -> the lazy nested view, and the
    reference consumers' access pattern on it (tools/api_time.py), at BASELINE configs[1] and configs[2].  Wall time of the
    Python call, host strings in, everything the call does inside (marshalling, upload, pack, scan, de-dup, copy-out)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import api_time
    out = {"unit": "bp*motifs/s", "definition": "region_bp x n_motifs / wall time of Scanner.scan_motifs(pwms) (host strings in, lazy "
           "MotifSites view out, de-dup on); writer = io/__init__.py:23-33's len(sites[idx]) / max(site.score) double loop, stats = stats.py:27-31, both run verbatim over the whole result",
           "reference_in_build_container": "profiles/archive/r04_api_time_reference.json (real Scanner.scan_motifs, configs[1], 8 threads)"}
    for key, name in (("configs1", "c2"), ("configs2", "c3")):
        m = api_time.measure(name)
        out[key] = {"value": m["value_api"], "scan_motifs_s": m["scan_motifs_s"], "scan_motifs_again_s": m["scan_motifs_again_s"],
                    "scanner_ctor_s": m["scanner_ctor_s"], "n_sites": m["n_sites"], "python_heap_bytes": m["scan_motifs_python_heap_bytes"],
                    # the reference's consumers, measured over EVERY region / motif (no extrapolation): iteration hands out one real list
                    # per motif, built on the first pass (rows_first_pass_s); the floor is the same loop over the reference's own lists
                    "rows_first_pass_s": m["rows_first_pass_s"],
                    "writer_ns_per_motif_region": m["writer_pattern"]["ns_per_motif_region"],
                    "writer_all_regions_s": m["writer_pattern"]["all_regions_s"], "writer_measured_over_all_regions": m["writer_pattern"]["measured_over_all_regions"],
                    "writer_on_reference_lists_ns_per_motif_region": m["writer_pattern_on_reference_lists_ns_per_motif_region"],
                    "stats_all_motifs_s": m["stats_pattern"]["all_motifs_s"], "vectorised_tables_s": m["vectorised_tables_s"]}
    return out


def end_to_end(a, wl, pw, world, dev, torch, dist, strand_mask=3):
    """Host ASCII in pinned memory -> hit arrays in pinned host memory, in batches of --batch-regions regions:
       pipelined  three stages of consecutive batches overlapped by the library's stream (ms_stream_*), hits copied out in the
                  compact 16-byte form (pipelined_25B: the int64/int64/f64/int8 arrays, 25 bytes per hit);
       serial     one batch at a time: upload + pack, scan, copy-out.
    Whole-job rates (max time over ranks)."""
    from motifscan_amd import _lib, dist as msdist
    pins, batches, cuts = [], [], []
    n_sets = len(wl["sets"])
    # the rank's main thread onto the GPU's NUMA node BEFORE it allocates its pinned input (first touch places the pages): the library's
    # policy -- multi-GPU nodes with more than one NUMA node, MS_NUMA_BIND=0/1 overrides (ms_numa.cpp); the stream's threads bind themselves
    numa_node = _lib.numa_bind_thread()
    t_pin = time.perf_counter()
    for k, (bases, offsets) in enumerate(wl["sets"]):
        pin = _lib.PinnedBuffer(max(bases.size, 1))
        pin.array[:bases.size] = bases
        pins.append(pin)
    t_pin = time.perf_counter() - t_pin
    for k, (bases, offsets) in enumerate(wl["sets"]):
        # batches grow from --batch-regions / 4 to --max-batch-regions at the start of a pass and shrink again at its end
        # (dist.batch_bounds): the pass begins with an upload nothing overlaps and ends with a copy-out nothing overlaps
        for r0, r1 in msdist.batch_bounds(len(offsets) - 1, a.batch_regions, ramp=not a.no_batch_ramp, max_batch=a.max_batch_regions,
                                          ramp_up=k == 0, ramp_down=k == n_sets - 1):
            cuts.append((k, r0, r1))
    for k, r0, r1 in cuts:
        offsets = wl["sets"][k][1]
        lo, hi = int(offsets[r0]), int(offsets[r1])
        batches.append((pins[k].array[lo:hi], np.ascontiguousarray(offsets[r0:r1 + 1] - lo)))
    units = float(wl["units"])

    each_pass = {}                                      # every timed pass of a leg by itself (ms): a leg's mean hides a single slow pass
    own = {}                                            # this rank's own seconds and process CPU seconds per leg (the per-rank report at N > 1)

    def timed(fn, passes, name=None):
        # (the cycle collector off inside the timed passes, as timeit does: this process has held tens of millions of Python objects -- the api leg's
        # sites -- and a full collection on the consumer's thread is a 30-ms hole in a 45-ms pass: the single slow passes of profiles/r06r_*.json.
        # Collected BEFORE the warm passes, not between them and the timed ones: what a collection frees -- results of the previous leg still held by
        # cycles -- goes back to the block caches and changes which blocks the next pass is handed; with the collection in between, the first timed
        # pass took 70-90 ms in half of the runs, profiles/r06z_offsets_ab.log)
        import gc
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        for _ in range(4):                              # warm: the device and pinned block caches take three passes to hold every size class a pass
            fn()                                        # asks for (tools/e2e_slow_pass_probe.py: 130, 65, 54, then 49 ms per pass; two warm passes left 54-58 ms passes in the timed four)
        if dist is not None:
            dist.barrier()
        c0 = os.times()
        t0 = time.perf_counter()
        hits = 0
        each = []
        for _ in range(passes):
            t1 = time.perf_counter()
            hits += fn()
            each.append(round((time.perf_counter() - t1) * 1e3, 2))
        if gc_was_on:
            gc.enable()
        if name:
            each_pass[name] = each
        if name:
            c1 = os.times()
            own[name] = ((time.perf_counter() - t0) / passes, (c1.user + c1.system - c0.user - c0.system) / passes)
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        u = torch.tensor([units * passes], dtype=torch.float64, device=dev)
        if dist is not None:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dist.all_reduce(u, op=dist.ReduceOp.SUM)
        return float(u.item()) / float(t.item()), float(t.item()) / passes * 1e3, hits // passes

    stages = {}

    def pipelined(packed):
        def run():
            n = 0
            st = stages.setdefault({12: "pipelined", 16: "pipelined_16B"}.get(packed, "pipelined_25B"), {})
            dev_ms = {"prefilter": 0.0, "fp64_stage": 0.0, "sort": 0.0, "finalize": 0.0, "scan_total": 0.0, "clock_mhz_sum": 0.0}
            for res in _lib.scan_stream(pw, iter(batches), strand_mask, 0, depth=2, packed=packed, stage_stats=st, host_pack=a.host_pack):
                n += res.n_hits                         # the arrays are already in pinned host memory at this point
                s_ = res.stats()
                for k_, f_ in (("prefilter", "ms_prefilter"), ("fp64_stage", "ms_exact"), ("sort", "ms_sort"), ("finalize", "ms_finalize"),
                               ("scan_total", "ms_total")):
                    dev_ms[k_] += s_[f_]
                dev_ms["clock_mhz_sum"] += s_["pf_clock_mhz"]          # 0 unless MS_MEASURE=1 MS_PF_CLOCK=1
                res.close()
            st["scan_device_ms"] = {k_: round(v_, 2) for k_, v_ in dev_ms.items()}
            return n
        return run

    # the same batches as ONE stream kept full over `reps` consecutive passes (a sweep over many region sets, configs[4]'s shape: the
    # ramp of small batches only at the very beginning and the very end, full-size batches in between): what a pass costs when its
    # first upload and last copy-out overlap the neighbouring passes' work
    def sustained_batches(reps):
        out = []
        for rep in range(reps):
            for k, (bases, offsets) in enumerate(wl["sets"]):
                for r0, r1 in msdist.batch_bounds(len(offsets) - 1, a.batch_regions, ramp=not a.no_batch_ramp, max_batch=a.max_batch_regions,
                                                  ramp_up=rep == 0 and k == 0, ramp_down=rep == reps - 1 and k == n_sets - 1):
                    lo, hi = int(offsets[r0]), int(offsets[r1])
                    out.append((pins[k].array[lo:hi], np.ascontiguousarray(offsets[r0:r1 + 1] - lo)))
        return out

    def sustained(reps):
        bl = sustained_batches(reps)

        def run():
            n = 0
            for res in _lib.scan_stream(pw, iter(bl), strand_mask, 0, depth=2, packed=12, host_pack=a.host_pack):
                n += res.n_hits
                res.close()
            return n
        return run

    # the reference CLI's data flow (cli/scan.py:43-48, 81-89): the INPUT regions' sites go to the writers, the CONTROL regions are only
    # counted (stats.py:29-31) -- one stream, control batches submitted counts-only (ms_stream_submit_counts_only)
    cli_batches = [(b, o, k > 0) for (b, o), (k, _, _) in zip(batches, cuts)]

    def pipelined_cli():
        n = 0
        st = stages.setdefault("pipelined_cli", {})
        for res, (_, _, counts_only) in zip(_lib.scan_stream(pw, iter(cli_batches), strand_mask, 0, depth=2, packed=12, stage_stats=st, host_pack=a.host_pack), cli_batches):
            if not counts_only:
                n += res.n_hits                         # in pinned host memory
            res.region_counts()
            res.close()
        return n

    def serial():
        n = 0
        for b, o in batches:
            sq = _lib.SeqSet(b, o)
            res = _lib.scan(pw, sq, strand_mask)
            res.hits(copy=False)
            n += res.n_hits
            res.close(); sq.close()
        return n

    passes = max(1, min(a.steps, 4))
    v_p12, ms_p12, hits = timed(pipelined(12), passes, "pipelined")
    v_cli, ms_cli, hits_cli = timed(pipelined_cli, passes, "pipelined_cli")
    v_p16, ms_p16, hits16 = timed(pipelined(16), passes, "pipelined_16B")
    v_p25, ms_p25, _ = timed(pipelined(False), passes)
    v_s, ms_s, _ = timed(serial, passes)
    reps = 4
    v_su, ms_su, hits_su = timed(sustained(reps), 1)
    v_su, ms_su = v_su * reps, ms_su / reps                     # timed() counts one call as one pass; the call holds `reps` of them
    for pin in pins:
        pin.close()
    # ---- the host side rank by rank: every rank's own pass time, the CPU seconds its process burnt per pass (stream threads
    # + Python), its stage waits, the time its pinned input took to allocate and fill, and where it was bound
    per_rank = None
    if dist is not None:
        st_p = stages.get("pipelined", {})
        mine = torch.tensor([own["pipelined"][0] * 1e3, own["pipelined"][1] * 1e3, own["pipelined_cli"][0] * 1e3, own["pipelined_cli"][1] * 1e3,
                             st_p.get("upload", {}).get("ms_work", 0.0), st_p.get("scan", {}).get("ms_work", 0.0), st_p.get("scan", {}).get("ms_wait_in", 0.0),
                             st_p.get("copy_out", {}).get("ms_work", 0.0), t_pin * 1e3, float(numa_node), float(len(os.sched_getaffinity(0)))],
                            dtype=torch.float64, device=dev)
        tab = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(tab, mine)
        tab = torch.stack(tab).cpu().numpy()
        units_rank = float(wl["units"])
        per_rank = {"ms_per_pass_pipelined": [round(float(x), 2) for x in tab[:, 0]], "cpu_ms_per_pass_pipelined": [round(float(x), 1) for x in tab[:, 1]],
                    "ms_per_pass_cli": [round(float(x), 2) for x in tab[:, 2]], "cpu_ms_per_pass_cli": [round(float(x), 1) for x in tab[:, 3]],
                    "value_8d_end_to_end_by_rank": [units_rank / (float(x) * 1e-3) for x in tab[:, 0]],
                    "stage_ms_last_pass_by_rank": {"upload_work": [round(float(x), 2) for x in tab[:, 4]], "scan_work": [round(float(x), 2) for x in tab[:, 5]],
                                                   "scan_wait_in": [round(float(x), 2) for x in tab[:, 6]], "copy_out_work": [round(float(x), 2) for x in tab[:, 7]]},
                    "pinned_input_alloc_and_fill_ms": [round(float(x), 1) for x in tab[:, 8]],
                    "numa_node_bound": [int(x) for x in tab[:, 9]], "cpus_allowed": [int(x) for x in tab[:, 10]],
                    "host_cpu_busy_fraction_of_box": float(tab[:, 1].sum() / max(tab[:, 0].max(), 1e-9) / (os.cpu_count() or 1)),
                    "host_cores": os.cpu_count()}
    return {"per_rank": per_rank, "ms_each_pass": each_pass, "host_pack": bool(a.host_pack), "numa_node_bound": numa_node, "pinned_input_alloc_and_fill_ms": round(t_pin * 1e3, 1),
            "pipelined": v_p12, "pipelined_cli": v_cli, "pipelined_16B": v_p16, "pipelined_25B": v_p25, "serial": v_s, "pipelined_sustained": v_su, "unit": "bp*motifs/s",
            "ms_per_pass": {"pipelined": ms_p12, "pipelined_cli": ms_cli, "pipelined_16B": ms_p16, "pipelined_25B": ms_p25, "serial": ms_s, "pipelined_sustained": ms_su},
            "hits_check_12B_vs_16B": bool(hits == hits16), "bytes_per_hit_on_the_link": {"pipelined": 12, "pipelined_cli": 12, "pipelined_16B": 16, "pipelined_25B": 25},
            "hits_out_per_pass_cli": int(hits_cli),
            "sustained_passes_per_stream": reps, "sustained_hits_check": bool(hits_su == hits * reps),
            "batches_per_pass_per_gpu": len(batches), "batch_regions": a.batch_regions, "max_batch_regions": a.max_batch_regions, "batch_sizes": [int(len(o) - 1) for _, o in batches], "batch_ramp": not a.no_batch_ramp, "hits_per_pass_per_gpu": int(hits),
            "stage_ms_last_pass": {k: {sk: {f: round(x, 2) for f, x in sv.items()} for sk, sv in v.items()} for k, v in stages.items()},
            "cu_partition": "off: the copy / pack kernels share the device with the scan (CU masks -- 1 CU of every 32 for the copy streams -- exist behind MS_MEASURE=1 MS_CU_PARTITION=1 and measured slower end to end, profiles/archive/r02_cu_partition_ab.log)",
            "definition": "SURVEY.md 8(d): host ASCII in pinned memory -> H2D + pack -> scan -> hit arrays (seq_idx, pos, score, strand) in pinned "
                          "host memory; 'pipelined' overlaps the three stages of consecutive batches (ms_stream) and moves 12 bytes per hit "
                          "(32-bit coord word region << shift | pos << 1 | strand + fp64 score: MS_STREAM_PACKED12, every batch of this workload fits it; 'pipelined_16B' = round 5's 64-bit coord word), 'pipelined_cli' is the reference CLI's own job (cli/scan.py:81-89: the input set's sites out, the control "
                          "set counted only -- stats.py:29-31 is all that reads it), 'pipelined_25B' the four plain arrays, 'serial' runs the stages of one batch after another; "
                          "'pipelined' opens and drains a stream for every pass (one pass = the job), 'pipelined_sustained' keeps ONE stream full over "
                          "several consecutive passes and divides by their number (a sweep over many region sets: the per-pass rate once the first "
                          "upload and the last copy-out overlap the neighbouring passes)"}


def main_sweep(a, world, rank, local_rank):
    """configs[4]: window sweeps.  c5 = host-streamed whole genome (strong scaling over the spans); c5shard = one GPU's 375 Mbp
    resident in HBM (round-1 comparison line)."""
    from motifscan_amd import dist as msdist, synth
    window, stride = synth.C5["window"], synth.C5["stride"]
    if a.workload == "c5":
        lens = synth.c5_chrom_lengths(a.genome_mbp * 1_000_000)
        vals, widths, cutoffs = synth.load_motif_set(synth.C5["n_pwms"])
        max_span = 375_000_000
        # span planning needs no GPU: a pure function of the lengths (the library's ms_sweep_spans, restated for the pre-GPU phase)
        spans_all = []
        first = 0
        for ch, L in enumerate(lens.tolist()):
            n_w = (L - window) // stride + 1 if L >= window else 0
            if not n_w:
                continue
            per = (max_span - window) // stride + 1
            n_sp = -(-n_w // per)
            for k in range(n_sp):
                k0, k1 = n_w * k // n_sp, n_w * (k + 1) // n_sp
                spans_all.append((ch, k0 * stride, (k1 - 1) * stride + window, first + k0, k1 - k0))
            first += n_w
        mine = msdist.span_shard(spans_all, rank, world)
        need = sorted({sp[0] for sp in mine})
        genome = synth.c5_genome(need, lens, workers=min(16, max(1, (os.cpu_count() or 1) // world)))
    else:
        wl = synth.workload("c5shard", rank=rank)

    import torch
    import torch.distributed as dist
    from motifscan_amd import _lib
    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise RuntimeError("bench.py needs an MI355X; there is no CPU fallback")
    backend = os.environ.get("MS_BENCH_BACKEND", "nccl")
    share = os.environ.get("MS_BENCH_SHARE_GPU") == "1"
    dev_index = local_rank % _lib.device_count() if share else local_rank
    torch.cuda.set_device(dev_index)
    _lib.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    if a.workload == "c5":
        assert _lib.sweep_spans(lens, window, stride, max_span) == spans_all       # the library's planner agrees
        P = len(widths)
        pw = _lib.PwmSet(vals, widths, cutoffs)
        pinned = {}
        for ch in need:                                # chromosomes in pinned host memory: uploads at link rate, overlapped
            pb = _lib.PinnedBuffer(len(genome[ch]))
            pb.array[:] = genome[ch]
            pinned[ch] = pb
        chroms = {ch: pb.array for ch, pb in pinned.items()}
        del genome
        counts = torch.zeros(P, dtype=torch.int64, device=dev)
        local_counts = torch.zeros(P, dtype=torch.int64, device=dev)
        my_units = float(sum(sp[4] for sp in mine)) * window * P
        modes = {"counts_only": (_lib.MS_STREAM_NO_HITS, False)}           # `value`
        if a.full:
            modes["hits_packed"] = (0, True)
        out = {}

        def one_pass(flags, packed):
            c = np.zeros(P, dtype=np.int64)
            sites = 0
            st = {"ms_prefilter": 0.0, "ms_total": 0.0, "n": 0, "stages": {}}
            for sp, res in _lib.sweep_stream(pw, chroms, window, stride, max_span, 3, flags, depth=2, spans=mine, packed=packed,
                                             stage_stats=st["stages"]):
                c += res.region_counts()
                sites += res.n_hits
                s = res.stats()
                st["ms_prefilter"] += s["ms_prefilter"]; st["ms_total"] += s["ms_total"]; st["n"] += 1
                res.close()
            counts.copy_(torch.from_numpy(c))
            local_counts.copy_(counts)
            if world > 1:
                dist.all_reduce(counts, op=dist.ReduceOp.SUM)
            return sites, st

        for mode, (flags, packed) in modes.items():
            t_w = time.perf_counter()
            n_warm = 0
            while n_warm < max(1, a.warmup) or (time.perf_counter() - t_w < a.min_warm_seconds and world == 1):
                one_pass(flags, packed)                # (N > 1: a fixed number of passes, every pass holds a collective)
                n_warm += 1
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pool0 = _lib.pool_stats()
            for _ in range(a.steps):
                sites, st = one_pass(flags, packed)
            pool1 = _lib.pool_stats()
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
            un = torch.tensor([my_units], dtype=torch.float64, device=dev)
            if world > 1:
                dist.all_reduce(el, op=dist.ReduceOp.MAX)
                dist.all_reduce(un, op=dist.ReduceOp.SUM)
            out[mode] = {"value": float(un.item()) * a.steps / float(el.item()), "ms_per_step": float(el.item()) / a.steps * 1e3,
                         "sites_per_step_per_gpu": int(sites), "spans_per_gpu": len(mine),
                         "prefilter_ms_per_step": st["ms_prefilter"], "device_ms_per_step": st["ms_total"],
                         "hbm_pool_timed": {k: pool1[k] - pool0[k] for k in ("hits", "misses", "driver_frees", "driver_ms")},
                         "stage_ms_last_pass": {sk: {f: round(x, 2) for f, x in sv.items()} for sk, sv in st["stages"].items()}}
        counts_check = None
        if a.full and world > 1:                       # the collective and the span shards, checked (last pass = hits_packed mode)
            gathered = [torch.zeros_like(local_counts) for _ in range(world)]
            dist.all_gather(gathered, local_counts)
            first_last = torch.tensor([float(mine[0][3]) if mine else -1.0, float(mine[-1][3] + mine[-1][4]) if mine else -1.0, float(len(mine))],
                                      dtype=torch.float64, device=dev)
            fl = [torch.zeros_like(first_last) for _ in range(world)]
            dist.all_gather(fl, first_last)
            fl = [x for x in torch.stack(fl).cpu().numpy().tolist() if x[2] > 0]
            n_windows_total = int(spans_all[-1][3] + spans_all[-1][4])
            counts_check = {"allreduce_equals_sum_of_rank_counts": bool(torch.equal(torch.stack(gathered).sum(0), counts)),
                            "max_windows_with_site": int(counts.max().item()),
                            "window_ranges_tile_the_sweep": bool(fl and fl[0][0] == 0 and fl[-1][1] == n_windows_total
                                                                 and all(fl[k][1] == fl[k + 1][0] for k in range(len(fl) - 1))),
                            "ranks_with_spans": len(fl)}
        if rank == 0:
            line = {"metric": "scanned bp*motifs per second (region_bp x n_motifs), both strands, p=1e-4 cutoffs",
                    "value": out["counts_only"]["value"], "unit": "bp*motifs/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                    "ms_per_step": out["counts_only"]["ms_per_step"], "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
                    "dtype": "f64 behind an fp6 x fp4 one-hot matrix-core pre-filter (exact f32 accumulate)", "data": "synthetic",
                    "config": {"workload": WORKLOAD_TEXT["c5"], "genome_bp": int(lens.sum()), "n_chroms": len(lens), "window": window,
                               "stride": stride, "n_windows_total": int(spans_all[-1][3] + spans_all[-1][4]), "n_pwms": P,
                               "max_span_bases": max_span, "spans_total": len(spans_all)},
                    "value_definition": "host-streamed END TO END (chromosomes in pinned host memory -> upload + pack | scan-once + hand-out | "
                                        "copy-out overlapped); units are reference-equivalent (window_bp x n_windows x n_motifs: the reference "
                                        "scans every base window / stride = 4 times, the sweep once). value = counts_only mode (per-motif window "
                                        "counts, what the enrichment statistics consume); hits_packed (--full) also copies every site to the host",
                    "modes": out}
            if counts_check is not None:
                line["counts_check"] = counts_check
            print(json.dumps(line), flush=True)
    else:
        P = wl["n_pwms"]
        pw = _lib.PwmSet(wl["pwm_values"], wl["widths"], wl["cutoffs"])
        genome = _lib.ResidentGenome({"chr": wl["genome"]})
        counts = torch.zeros(P, dtype=torch.int64, device=dev)

        def step():
            res = _lib.scan_sweep(pw, genome, "chr", 0, len(wl["genome"]), window, stride, 3)
            st = res.stats()
            counts.copy_(torch.as_tensor(_DevicePtr(res.region_counts_device_ptr(), P), device=dev))
            torch.cuda.current_stream().synchronize()
            res.close()
            if world > 1:
                dist.all_reduce(counts, op=dist.ReduceOp.SUM)
            return st

        t_w = time.perf_counter()
        n_warm = 0
        while n_warm < a.warmup or (time.perf_counter() - t_w < a.min_warm_seconds and world == 1):
            step()
            n_warm += 1
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = [step() for _ in range(a.steps)]
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        un = torch.tensor([float(wl["units"])], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(el, op=dist.ReduceOp.MAX)
            dist.all_reduce(un, op=dist.ReduceOp.SUM)
        if rank == 0:
            k = len(stats)
            line = {"metric": "scanned bp*motifs per second (region_bp x n_motifs), both strands, p=1e-4 cutoffs",
                    "value": float(un.item()) * a.steps / float(el.item()), "unit": "bp*motifs/s (reference-equivalent units)", "n_gpus": world,
                    "steps": a.steps, "warmup": a.warmup, "ms_per_step": float(el.item()) / a.steps * 1e3, "higher_is_better": True,
                    "scaling": "weak", "vs_baseline": None, "dtype": "f64 behind an fp6 x fp4 one-hot matrix-core pre-filter (exact f32 accumulate)",
                    "data": "synthetic", "config": {"workload": WORKLOAD_TEXT["c5shard"], "n_pwms": P, "windows_per_gpu": wl["n_regions"]},
                    "stage_ms_per_scan": {q: sum(s[q] for s in stats) / k for q in ("ms_prefilter", "ms_exact", "ms_sort", "ms_finalize", "ms_total")},
                    "hits_per_scan": sum(s["n_hits"] for s in stats) / k}
            print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
