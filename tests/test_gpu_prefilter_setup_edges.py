"""
The set-up of a pre-filter pass at its edges: sequence staging, the one-hot array, the work hand-out.  prefilter_f6_kernel<2, *> builds, per
wave and pass of 128 window starts, a one-hot array of 160 entries from 168 staged bases, prefetches the next pass's words -- of its unit, or
of the unit the hand-out's counter gave it -- and clears or drops what is non-ACGT.  As in tests/test_gpu_prefilter_candidates.py the whole
candidate list (_lib.scan_candidates) must BE the model's flags (prefilter_model.model_flags, through prefilter_cases.build): for every
base, table group and field the device's bit equals the model's; device <= model only in dead windows under skip_alln, as there.

The cases, each in the parked and in the dense form (MS_PF_DENSE), both strands:
    len-N       prefixes of the `small` text of N bases around 32 (a lane half), 128 (a pass), 160 (the array's entries) and 168 (the bases
                a pass needs), and 255 ... 257
    unit±       MS_PF_MAX_BLOCKS=1, sixteen waves: a first launch reports wave_passes; inputs of ONE unit (128 x wave_passes bases) and of
                FIFTEEN units, each -1 / +0 / +1 base -- the fifteen-unit launches report the same wave_passes again (asserted), so the
                input ends one base before, on and one base behind a unit's last pass
    counter     MS_PF_MAX_BLOCKS=1: the largest input the launch scans without the counters and the smallest it scans with them, from the
                first launch's blocks and pass size (prefilter_cases.counter_point) and asserted on what the launches report; with the
                counters one wave takes some thirty units through the atomic.  NOTE: these two inputs are 131 072 and 131 073 bases -- with
                sixteen waves the counter hand-out begins above 1024 passes (launch_shape, ms_scan_geom.cpp), so no input of at most
                100 000 bases reaches it; every other case stays far below that size.
    nruns       runs of N that begin and that end 63, 64, 127, 128, 159, 160, 167 and 168 bases behind a pass's first; runs of exactly
                31, 32 and 33 N (none, one and two dead windows) at four phases; a run that ends with the input's last base, and one that
                ends three bases before it, in its last code word -- on the `small` set (dead windows dropped) and on `alln`, whose motif
                at cutoff 0.0 switches the dead-window rule off
"""
import numpy as np
import pytest

import prefilter_cases as pc
import prefilter_model as pm
from motifscan_amd import _lib

pytestmark = pytest.mark.gpu

ENV = ("MS_PF_DENSE", "MS_PF_RARE_CAP", "MS_PF_MAX_BLOCKS", "MS_PF_LDS_BUDGET", "MS_PF_PAIR", "MS_RESCORE_SORTED_MIN", "MS_NO_PREDICT")
FORMS = {"parked": "0", "dense": "1"}
LENGTHS = (1, 31, 32, 33, 127, 128, 129, 159, 160, 161, 167, 168, 169, 255, 256, 257)
RUN_OFFSETS = (63, 64, 127, 128, 159, 160, 167, 168)
DEAD_RUNS = (31, 32, 33)
DEAD_PHASES = (0, 1, 96, 100)
SLOT = 384                      # bases per run: a pass in front of the pass the offsets count from, and one behind


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


def _case(form, set_name="small", prefix=None, seq=("full", 0), text=None, env=None, skip_alln=1):
    e = {"MS_PF_DENSE": FORMS[form]}
    e.update(env or {})
    c = {"kind": "setup", "kernel": form, "strand": 3, "set": set_name, "seq": seq, "prefix": prefix, "env": e, "budget": 70 * 1024, "pair": True,
         "expect": {"wide": 0, "dense": int(form == "dense"), "pass_windows": 128, "skip_alln": skip_alln}}
    if text is not None:
        c["text"] = text
    return c


def n_run_text(set_name, tail):
    """runs of N in slots of SLOT bases (each slot starts on a pass boundary; offsets count from its second pass), the filler the planted
    consensus sequences of the set's text; then a run of nine N and `tail`"""
    fill = "".join(ch for ch in pc.sequence(set_name)[:6000] if ch in "ACGT")
    at = [0]

    def take(n):
        out = "".join(fill[(at[0] + i) % len(fill)] for i in range(n))
        at[0] += n
        return out

    runs = [(o, 5) for o in RUN_OFFSETS] + [(o - 5, 5) for o in RUN_OFFSETS] + [(p, n) for n in DEAD_RUNS for p in DEAD_PHASES]
    s = []
    for start, n in runs:
        slot = list(take(SLOT))
        slot[128 + start:128 + start + n] = "N" * n
        s.append("".join(slot))
    return "".join(s) + take(100) + "N" * 9 + tail


def _set_env(monkeypatch, case):
    monkeypatch.setenv("MS_MEASURE", "1")
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    if "text" in case:                                         # a text of this file's making, through prefilter_cases.build all the same
        monkeypatch.setattr(pc, "case_text", lambda c: c["text"])


def _launch(case, pwms, text):
    sq = _lib.SeqSet(text.encode(), np.array([0, len(text)], dtype=np.int64))
    rec, geom, cap = _lib.scan_candidates(pwms, sq, case["strand"])
    sq.close()
    return rec, geom, cap


def geometry(monkeypatch, case):
    """what the launch of the case reports (no model: the case is only asked for its geometry)"""
    _set_env(monkeypatch, case)
    mats, cut = pc.motif_set(case["set"])
    vals, widths = pc.flat(mats)
    return _launch(case, _lib.PwmSet(vals, widths, cut), pc.case_text(case))[1]


def _scan(monkeypatch, case):
    _set_env(monkeypatch, case)
    b = pc.build(case, _lib)
    return (b,) + _launch(case, b["pwms"], b["text"])


def check(monkeypatch, name, case, expect=None):
    """the candidate list of the case against the model, bit by bit; returns the launch's geometry"""
    b, rec, geom, cap = _scan(monkeypatch, case)
    plan, n_bases = b["plan"], len(b["text"])
    n_groups = plan["group_fields"].shape[0]
    for k, v in {**case["expect"], **(expect or {})}.items():
        assert geom[k] == v, f"{name}: the launch has {k} = {geom[k]}, the case is about {v} ({geom})"
    assert len(rec) <= cap and len(rec) >= geom["cand_static"]
    got, t = pm.decode_records(rec, n_groups, n_bases)
    assert t["bad_g"] == 0 and t["bad_group"] == 0 and t["repeated"] == 0, f"{name}: {t} among {len(rec)} slots, {n_bases} bases, {n_groups} groups ({geom})"
    occ = pm.occupied_mask(plan)
    assert not (got & ~occ[:, None]).any(), f"{name}: a record flags an empty field"
    lower, upper = pc.expected_flags(plan, b["model"], b["isn"], False, bool(geom["skip_alln"]))
    print(f"{name}: {n_bases} bases, {n_groups} groups, {len(rec)} slots, {int(np.count_nonzero(got))} records, model {int(np.count_nonzero(upper))} "
          f"({int(np.count_nonzero(upper & ~lower))} in dead windows); {geom}")
    for diff, what in ((got & ~upper, "the device flags what the model does not"), (lower & ~got, "the device misses a model flag"),
                       (got & ~lower, "the device flags in a dead window")):
        if diff.any():
            q, g = (int(v[0]) for v in np.nonzero(diff))
            pytest.fail(f"{name}: {what}: group {q} g {g} (g mod 128 = {g % 128}) device {int(got[q, g]):#06x} model {int(upper[q, g]):#06x}; "
                        f"{int(np.count_nonzero(diff))} (g, group) pairs differ in this way; {geom}")
    return geom


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("n", LENGTHS)
def test_input_lengths(monkeypatch, n, form):
    check(monkeypatch, f"len-{n}-{form}", _case(form, prefix=n))


def _one_block(form, n, fill_to=0):
    return _case(form, prefix=n, seq=("full", fill_to), env={"MS_PF_MAX_BLOCKS": "1"})


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("d", (-1, 0, 1))
def test_lengths_around_a_unit(monkeypatch, d, form):
    fill = 24000
    g0 = geometry(monkeypatch, _one_block(form, 20000, fill))
    wp = g0["wave_passes"]
    assert g0["blocks_per_tile"] == 1 and g0["counter_used"] == 0 and wp > 1, g0
    unit = g0["pass_windows"] * wp
    assert 15 * unit + 1 <= fill - 200
    check(monkeypatch, f"unit{d:+d}-{form}", _one_block(form, unit + d, fill), {"blocks_per_tile": 1, "counter_used": 0})
    # fifteen of the sixteen waves take a unit of the same wave_passes: the last of them ends one base before, on, one base behind its unit's end
    check(monkeypatch, f"15units{d:+d}-{form}", _one_block(form, 15 * unit + d, fill), {"blocks_per_tile": 1, "counter_used": 0, "wave_passes": wp})


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("counters", (0, 1))
def test_counter_hand_out_threshold(monkeypatch, counters, form):
    g0 = geometry(monkeypatch, _one_block(form, 4096))
    assert g0["blocks_per_tile"] == 1, g0
    point = pc.counter_point(g0["blocks_per_tile"], g0["pass_windows"])        # the largest input without the counters
    n = point + counters
    geom = check(monkeypatch, f"counter{counters}-{form}", _one_block(form, n, point + 400), {"blocks_per_tile": 1, "counter_used": counters})
    if counters:
        n_units = -(-(-(-n // geom["pass_windows"])) // geom["wave_passes"])
        assert n_units >= 8 * 16, (geom, n_units)                                # several units per wave, all but the first through the atomic


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("set_name", ("small", "alln"))
@pytest.mark.parametrize("tail", ("", "ACG"))
def test_runs_of_n(monkeypatch, tail, set_name, form):
    text = n_run_text(set_name, tail)
    assert len(text) <= 100000 and text.endswith("N" * 9 + tail)
    case = _case(form, set_name=set_name, seq=("nruns", len(tail)), text=text, skip_alln=int(set_name != "alln"))
    check(monkeypatch, f"nruns-{set_name}-{len(tail)}-{form}", case)
