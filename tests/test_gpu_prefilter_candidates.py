"""
prefilter_f6_kernel against its model, record by record.  tests/test_host_cabi.py proves on the CPU that the PLAN -- the physical fp6 operand
image -- never loses a reference hit, through a numpy model of the integer pre-filter; the scan's own tests see the kernel only through the
candidates that are also hits.  Here the kernel's whole output, the candidate list (ms_debug_scan_candidates), must BE the model's
(prefilter_model.model_flags): for every base g of the input, every table group and every field the device's bit equals the model's.

One exception: where no motif of the plan can report a window of non-ACGT bases only (PfArgs::skip_alln), the kernel drops a window whose next
32 bases (64 in a tile with row tiles of 3 or 4 k-blocks) are all non-ACGT unseen -- "dead" (scan_pass / scan_pass2).  There the device must
flag nothing, so it is held to device <= model, and the model bits that leaves out are printed (only the shortest motifs, whose bias alone is
>= 0, have any).  The `alln` cases plan a motif at cutoff 0.0, which switches the rule off: dead windows then fall under the exact contract.

Beside the bits: no record names a base or a group outside the scan, none flags an empty field (the 64-column motif of the wide set sits on
the all-fp64 path and in no record), no (g, group) comes twice, every slot is a valid record or empty, and the geometry the launch reports is
the regime the case names.  prefilter_cases.py describes the motif sets, the text and the cases; what each case puts in front of the kernel
is asserted without a GPU in tests/test_prefilter_model_host.py and again here, on what was compared.
"""
import numpy as np
import pytest

import prefilter_cases as pc
import prefilter_model as pm
from motifscan_amd import _lib

pytestmark = pytest.mark.gpu

ENV = ("MS_PF_DENSE", "MS_PF_RARE_CAP", "MS_PF_MAX_BLOCKS", "MS_PF_LDS_BUDGET", "MS_PF_PAIR", "MS_RESCORE_SORTED_MIN", "MS_NO_PREDICT")


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


def _set_env(monkeypatch, env):
    monkeypatch.setenv("MS_MEASURE", "1")
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _first_difference(b, geom, got, diff, what):
    """(group, field, motif, width, g, g mod 128, lane, operand, model acc) of the first of the bits `diff` in which the device is wrong"""
    plan = b["plan"]
    q, g = (int(v[0]) for v in np.nonzero(diff))
    n = int(np.flatnonzero([(int(diff[q, g]) >> k) & 1 for k in range(16)])[0])
    m = int(plan["group_fields"][q, n])
    q0, h = pm.row_tiles(plan)[q]
    pw = geom["pass_windows"]
    return (f"{what}: group {q} (row tile from group {q0}, {'paired' if plan['group_paired'][q] else 'plain'}, {int(plan['group_kb'][q])} instructions) field {n} "
            f"motif {m} width {int(b['widths'][m]) if m >= 0 else 0} g {g} g mod 128 {g % 128} lane {g % 32 + 32 * h} operand {(g % pw) // 32} "
            f"model acc {pm.model_acc(plan, b['codes'], b['isn'], q, n, g)}: device bit {(int(got[q, g]) >> n) & 1}, "
            f"expected {1 - ((int(got[q, g]) >> n) & 1)} ({int(np.count_nonzero(diff))} (g, group) pairs differ in this way)")


def check_case(monkeypatch, name):
    case = pc.CASES[name]
    _set_env(monkeypatch, case["env"])
    b = pc.build(case, _lib)
    plan, n_bases = b["plan"], len(b["text"])
    n_groups = plan["group_fields"].shape[0]
    raw = b["text"].encode()
    sq = _lib.SeqSet(raw, np.array([0, n_bases], dtype=np.int64))
    rec, geom, cap = _lib.scan_candidates(b["pwms"], sq, case["strand"])
    # the regime
    for k, v in case["expect"].items():
        assert geom[k] == v, f"{name}: the launch has {k} = {geom[k]}, the case is about {v} ({geom})"
    assert geom["n_tiles"] == plan["n_tiles"] and (case["kind"] != "tiles" or geom["n_tiles"] >= 2), (name, geom)
    assert geom["skip_alln"] == case["expect"].get("skip_alln", 1)
    if case["kind"] == "counter":
        n_units = -(-(-(-n_bases // geom["pass_windows"])) // geom["wave_passes"])
        assert geom["counter_used"] == 1 and n_units > 16 * geom["blocks_per_tile"] * geom["n_tiles"], (name, geom, n_units)
    # the list: every slot empty or valid, nothing twice
    assert len(rec) <= cap and len(rec) >= geom["cand_static"]
    got, t = pm.decode_records(rec, n_groups, n_bases)
    bad = [(int(r >> np.uint64(30)), int((r >> np.uint64(16)) & np.uint64(0x3FFF)), int(r & np.uint64(0xFFFF))) for r in rec
           if (r & np.uint64(0xFFFF)) and ((r >> np.uint64(30)) >= n_bases or ((r >> np.uint64(16)) & np.uint64(0x3FFF)) >= n_groups)][:1]
    assert t["bad_g"] == 0 and t["bad_group"] == 0 and t["repeated"] == 0, \
        f"{name}: {t} among {len(rec)} slots of a scan of {n_bases} bases and {n_groups} groups; first (g, group, flags) outside it: {bad}"
    occ = pm.occupied_mask(plan)
    assert not (got & ~occ[:, None]).any(), f"{name}: a record flags an empty field"
    # the bits
    lower, upper = pc.expected_flags(plan, b["model"], b["isn"], bool(geom["wide"]), bool(geom["skip_alln"]))
    left_out = int(np.count_nonzero(upper & ~lower))
    tal = pc.tally(plan, b["model"], b["isn"], case, b["widths"])
    print(f"{name}: {n_bases} bases, {n_groups} groups, {len(rec)} slots ({t['empty']} empty), {int(np.count_nonzero(got))} records; dead windows leave "
          f"out {left_out} model records; {geom}; {({k: v for k, v in tal.items() if k != 'forms'})}")
    for diff, what in ((got & ~upper, "the device flags what the model does not"), (lower & ~got, "the device misses a model flag"),
                       (got & ~lower, "the device flags in a dead window")):
        assert not diff.any(), _first_difference(b, geom, got, diff, f"{name}: {what}")
    assert not pc.unmet(case, tal), pc.unmet(case, tal)
    sq.close()


@pytest.mark.parametrize("name", [n for n, c in pc.CASES.items() if c["kind"] != "tail"])
def test_candidate_list_is_the_model(monkeypatch, name):
    check_case(monkeypatch, name)


@pytest.mark.parametrize("kernel", sorted(pc.KERNELS))
def test_tail_prefixes(monkeypatch, kernel):
    """prefixes of the basic text: `live`, the last partial pass and launch_prefilter's block clamp decide what is flagged"""
    for n in pc.TAIL_PREFIXES:
        check_case(monkeypatch, f"tail-{kernel}-{n}")
