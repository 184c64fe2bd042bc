"""Every knob-selected variant of the engine held to the oracle.

The engine picks kernels, template instantiations and grid shapes through developer knobs: RM_* environment variables read
by the library (getenv in radio-sim_amd/csrc/).  VARIANTS below has one row per setting: its knobs, when the library reads
them (once per process -- a `static const` -- or per context, call, tick, batch or launch), the scenarios that run under it
(tests/multi/variant_worker.py) and its selection proof: the kernels that must and must not have run in a profiled rerun of one
scenario, so that a variant that silently takes the default path fails.  Rows that change only a grid size or a run length say
"launch shape only" and pick scenarios where that value changes the grid.

Each knob read once per process gets a child process of its own; the rows read per call share one child, which changes
os.environ between runs and makes a new Engine for every scenario.  The children run one at a time, each under a time limit;
this process never opens the GPU (it builds the library and runs the oracle).  A child that ends abnormally (signal, time
limit) stops every later variant test before it starts a process.

test_every_knob_has_a_row (no GPU) keeps the table complete: every getenv("RM_...") of the library is a row or exempt.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "multi", "variant_worker.py")

# when the library reads each knob: "once" (per process: a static const), "context" (at rm_create), "call" (per API call,
# tick, batch or launch)
READ = {
    "RM_FRAME_TICK": "once", "RM_AIR_LISTS": "once", "RM_BATCH_FRAMES": "once", "RM_BATCH_SHARDS": "once",
    "RM_FRAMES_CAND": "once", "RM_FR_FLAT_MAX": "once", "RM_FR_NO_SHADOW": "once", "RM_PACK_WGS": "once",
    "RM_NO_REC32": "once", "RM_NO_ZERO_COPY": "once", "RM_HOST_LINK_RSSI": "once", "RM_CHANNEL_ORDER": "once",
    "RM_RESORT_AFTER": "once", "RM_EV_FUSE": "once", "RM_EV_SHARE": "once", "RM_EV_EMIT_LDS": "once",
    "RM_GROUP_NO_RCCL": "once", "RM_GRAPH": "context",
    "RM_FILTER": "call", "RM_WG_RPT": "call", "RM_NO_SHADOW_TABLE": "call", "RM_NO_ONE_LAUNCH": "call",
    "RM_EXACT_GRID": "call", "RM_SINR_GX": "call", "RM_SINR_SCAN": "call", "RM_SINR_FRAMES": "call",
    "RM_FILTER_TICKS_PER_WG": "call", "RM_FILTER_GROUP": "call", "RM_FPW": "call", "RM_REORDER_RUN": "call",
    "RM_DENSE_TICK": "call", "RM_DENSE_LAZY": "call", "RM_NEAR_LISTS": "call", "RM_OV_PAIR_CAP": "call",
    "RM_OV_PAIRS_WGS": "call", "RM_OV_EXACT_GX": "call", "RM_RANK_FRAMES": "call", "RM_RANK_MARGIN": "call",
    "RM_SINR_ACC": "call", "RM_TICK_XCD_MAP": "call",
}

# knobs that select no variant of what the engine computes
EXEMPT = {
    "RM_RCCL_LIB": "the path of the RCCL library to bind, no code path of the engine",
    "RM_LIBRARY": "the path of the library the Python binding loads (a diagnostic build)",
    "RM_HOST_TIMING": "host-side timing printed to stderr; nothing launched changes",
    "RM_GROUP_NO_RCCL": "one GPU: a group of one member uses no RCCL either way (tests/test_gpu_group.py runs both)",
}

LONE = ["udgm_lone", "sinr_lone"]
# (the dropped-tick scenario runs in the SINR medium's scan form; with the per-receiver lists a first tick of ten frames is
# reported dropped at this capacity and layout -- open: tests/test_gpu_logdist.py::test_sinr_lists_after_a_dropped_tick holds
# the lists' form on its own layout)


def row(env, scenarios, proof=None, present=(), absent=(), shape=False, covered_by=None, note="", proofs=()):
    knobs = dict(kv.split("=", 1) for kv in env.split())
    proofs = list(proofs) + ([(proof, list(present), list(absent))] if proof else [])
    return dict(env=env, knobs=knobs, scenarios=list(scenarios), proofs=proofs, shape=shape, covered_by=covered_by, note=note,
                read="once" if any(READ[k] in ("once", "context") for k in knobs) else "call")


# One row per setting.  proof: the scenario rerun under rm_profile_enable; present / absent: kernel names (up to the template
# arguments) that must / must not be among its launches (proofs: several such triples).  shape: "launch shape only" (the value changes a grid or a run length).
VARIANTS = [
    row("", ["udgm_lone", "transmit", "logdist_batch", "big_batch", "sinr_lone", "sinr_batch", "sinr_overlap", "overflow", "gathered",
             "gathered_spatial", "gathered_overlap", "events", "events_rings"],
        proofs=[("udgm_lone", ["k_tick_frames"], ["k_filter", "k_exact"]),
                ("sinr_lone", ["k_tick_frames_scan", "k_sinr_scan"], ["k_filter", "k_frames_cand", "k_tick_frames_sinr"]),
                ("logdist_batch", ["k_exact_batch", "k_filter_wg_batch"], ["k_tick_frames_batch", "k_near_lists"]),
                ("big_batch", ["k_near_lists"], []),
                ("sinr_batch", ["k_sinr_acc_batch"], ["k_sinr_batch"]),
                ("gathered", ["k_rank_frames"], []),
                ("transmit", [], ["k_tick_frames"]),
                ("events_rings", ["k_ev_append_select"], [])],
        note="the defaults: every scenario; the baseline the selection proofs of the other rows differ from"),
    # ---- the filter's form
    row("RM_FILTER=wg", ["logdist_batch", "sinr_lone", "gathered"], proof="logdist_batch", present=["k_filter_wg_batch"], absent=["k_filter"]),
    row("RM_FILTER=wg RM_WG_RPT=4", ["logdist_batch", "gathered"], proof="logdist_batch", present=["k_filter_wg_batch"]),
    row("RM_FILTER=wg RM_WG_RPT=2", ["logdist_batch", "gathered"], proof="logdist_batch", present=["k_filter_wg_batch"]),
    row("RM_FILTER=grid", ["udgm_lone", "logdist_batch", "sinr_lone"], proof="logdist_batch", present=["k_filter_wg_batch"],
        note="a batch keeps the two-level filter whatever the knob says; lone ticks take the one-launch form: see the next row"),
    row("RM_FILTER=grid RM_SINR_FRAMES=0", ["sinr_lone"], proof="sinr_lone", present=["k_filter"],
        absent=["k_filter_wg", "k_frames_cand", "k_tick_frames_sinr"]),
    row("RM_NO_SHADOW_TABLE=1", ["logdist_batch", "sinr_lone", "gathered"], note="the shadowing by hash per link: a template argument"),
    row("RM_NO_ONE_LAUNCH=1", ["transmit"], proof="transmit", present=["k_tick_frames"],
        note="rm_transmit through the tick path instead of k_transmit_one (which is not profiled)"),
    # ---- the exact stage's grid
    row("RM_EXACT_GRID=1", ["logdist_batch", "gathered", "sinr_batch"], shape=True),
    row("RM_EXACT_GRID=7", ["logdist_batch", "gathered", "sinr_batch"], shape=True),
    row("RM_EXACT_GRID=256", ["logdist_batch", "gathered", "sinr_batch"], shape=True),
    # ---- lone ticks: one launch or three, the SINR medium by scan or by lists
    row("RM_FRAME_TICK=0", ["udgm_lone", "sinr_lone"], proof="udgm_lone", present=["k_filter"], absent=["k_tick_frames"]),
    row("RM_SINR_SCAN=0 RM_AIR_LISTS=0", ["sinr_lone"], proof="sinr_lone", absent=["k_sinr_scan", "k_tick_frames_scan"]),
    row("RM_FILTER=wg RM_FRAMES_CAND=0", ["sinr_lone"], note="the per-frame candidate kernel only serves the sweep of a SINR tick "
        "by lists; see the row with RM_SINR_FRAMES=0"),
    row("RM_FILTER=wg RM_FRAMES_CAND=0 RM_SINR_FRAMES=0", ["sinr_lone"], proof="sinr_lone", present=["k_filter_wg"],
        absent=["k_frames_cand", "k_tick_frames"]),
    row("RM_FR_FLAT_MAX=0", ["udgm_lone", "sinr_lone"], shape=True, note="every group through the level-1 boxes: a template argument"),
    row("RM_FR_NO_SHADOW=1", ["sinr_lone", "overflow"], note="the one-launch SINR tick without the shadowing table: a template argument"),
    row("RM_SINR_FRAMES=0", ["sinr_lone"], proof="sinr_lone", absent=["k_tick_frames_sinr", "k_sinr_scan"]),
    row("RM_SINR_FRAMES=0 RM_FILTER=wg", ["sinr_lone"], proof="sinr_lone", present=["k_frames_cand"],
        absent=["k_tick_frames_sinr", "k_sinr_scan"]),
    row("RM_SINR_SCAN=0", ["sinr_lone"], proof="sinr_lone", present=["k_tick_frames_sinr"], absent=["k_sinr_scan"]),
    row("RM_TICK_XCD_MAP=0", LONE, shape=True, covered_by="tests/test_gpu_logdist.py"),
    # ---- batches
    row("RM_FILTER_TICKS_PER_WG=3", ["logdist_batch", "gathered"], shape=True),
    row("RM_FPW=3", ["logdist_batch", "sinr_batch", "gathered"], shape=True),
    row("RM_FPW=200", ["logdist_batch", "sinr_batch", "gathered"], shape=True),
    row("RM_REORDER_RUN=0", ["logdist_batch", "sinr_batch", "gathered"], shape=True),
    row("RM_REORDER_RUN=6", ["logdist_batch", "sinr_batch", "gathered"], shape=True),
    row("RM_REORDER_RUN=3 RM_FPW=5", ["logdist_batch", "sinr_batch", "gathered"], shape=True),
    row("RM_SINR_GX=5 RM_SINR_ACC=0", ["sinr_batch"], shape=True, note="k_sinr_batch runs on the per-receiver lists only"),
    row("RM_SINR_GX=1 RM_SINR_ACC=0", ["sinr_batch"], shape=True, note="one workgroup per shard: the waves stride"),
    row("RM_SINR_ACC=0", ["sinr_batch", "gathered_overlap"], proof="sinr_batch", present=["k_sinr_batch"], absent=["k_sinr_acc_batch"]),
    row("RM_NEAR_LISTS=0", ["big_batch"], proof="big_batch", absent=["k_near_lists"]),
    row("RM_NEAR_LISTS=2 RM_WG_RPT=4", ["logdist_batch", "gathered"], proof="logdist_batch", present=["k_near_lists"],
        covered_by="tests/test_gpu_batch.py"),
    row("RM_NEAR_LISTS=2 RM_WG_RPT=4 RM_FILTER_TICKS_PER_WG=5 RM_FILTER_GROUP=1", ["logdist_batch"], proof="logdist_batch",
        present=["k_filter_wg_group"]),
    row("RM_NEAR_LISTS=2 RM_WG_RPT=4 RM_FILTER_TICKS_PER_WG=40 RM_FILTER_GROUP=1", ["logdist_batch"], proof="logdist_batch",
        present=["k_filter_wg_group"]),
    row("RM_FILTER_GROUP=0 RM_NEAR_LISTS=2 RM_WG_RPT=4 RM_FILTER_TICKS_PER_WG=5", ["logdist_batch", "big_batch"], proof="logdist_batch",
        present=["k_near_lists", "k_filter_wg_batch"], absent=["k_filter_wg_group"],
        note="against the two rows before: the grouped filter needs the lists and several ticks per workgroup to be a choice"),
    row("RM_BATCH_FRAMES=1", ["logdist_batch", "gathered", "gathered_spatial"], proof="logdist_batch",
        present=["k_tick_frames_batch"], absent=["k_exact_batch"]),
    row("RM_BATCH_SHARDS=8", ["gathered"], shape=True),
    row("RM_BATCH_SHARDS=16", ["gathered"], shape=True),
    row("RM_BATCH_SHARDS=32", ["gathered"], shape=True),
    row("RM_PACK_WGS=8", ["udgm_lone"], shape=True, note="the last tick's links outnumber eight workgroups' lanes"),
    row("RM_RANK_FRAMES=0", ["gathered", "gathered_spatial", "gathered_overlap"], proof="gathered", absent=["k_rank_frames"],
        covered_by="tests/test_gpu_sharded.py"),
    row("RM_RANK_MARGIN=0", ["gathered_overlap"], note="exact while no receiver moves between batches (no move here): the margin "
        "only keeps frames for receivers that move while they are on the air"),
    row("RM_RANK_MARGIN=100000", ["gathered_overlap"], note="every frame kept"),
    # ---- SINR batches whose frames outlive their ticks
    row("RM_OV_PAIR_CAP=4096", ["sinr_overlap", "gathered_overlap"], covered_by="tests/test_gpu_overlap.py"),
    row("RM_OV_PAIRS_WGS=1", ["sinr_overlap"], shape=True, note="one workgroup strides over every (tick, frame) item"),
    row("RM_OV_EXACT_GX=1", ["sinr_overlap"], shape=True, note="one workgroup per shard"),
    # ---- the dense tick
    row("RM_DENSE_TICK=1", ["udgm_lone", "logdist_batch"], covered_by="tests/test_gpu_dense.py"),
    row("RM_DENSE_TICK=0", ["udgm_lone", "logdist_batch"], covered_by="tests/test_gpu_dense.py"),
    row("RM_DENSE_LAZY=0", ["udgm_lone"], covered_by="tests/test_gpu_dense.py"),
    # ---- host side, tables, contexts
    row("RM_NO_REC32=1", ["udgm_lone", "logdist_batch", "sinr_lone"]),
    row("RM_NO_ZERO_COPY=1", ["udgm_lone"]),
    row("RM_HOST_LINK_RSSI=1", ["udgm_lone"]),
    row("RM_CHANNEL_ORDER=0", ["sinr_lone", "sinr_batch", "gathered"]),
    row("RM_RESORT_AFTER=0", ["sinr_lone"], note="tick 3's move sorts the table again"),
    row("RM_GRAPH=1", ["udgm_lone", "logdist_batch", "sinr_lone"]),
    # ---- the reception stage
    # (events_rings: each of the four reads the link pool through its own copy of the wrap arithmetic)
    row("RM_EV_FUSE=0", ["events", "events_rings"], proof="events_rings", present=["k_ev_select"], absent=["k_ev_append_select"]),
    row("RM_EV_SHARE=0", ["events", "events_rings"]),
    row("RM_EV_SHARE=1", ["events", "events_rings"]),
    row("RM_EV_EMIT_LDS=0", ["events", "events_rings"]),
]

# settings the table must hold beyond tools/knob_sweep.sh's K array (the sweep's own are read from the script)
REQUIRED_EXTRA = {"", "RM_BATCH_FRAMES=1", "RM_BATCH_SHARDS=8", "RM_BATCH_SHARDS=16", "RM_BATCH_SHARDS=32", "RM_PACK_WGS=8",
                  "RM_OV_PAIRS_WGS=1", "RM_OV_EXACT_GX=1", "RM_CHANNEL_ORDER=0", "RM_NEAR_LISTS=0", "RM_SINR_GX=1 RM_SINR_ACC=0",
                  "RM_SINR_GX=5 RM_SINR_ACC=0", "RM_RANK_MARGIN=0", "RM_RANK_MARGIN=100000",
                  "RM_FILTER=wg RM_FRAMES_CAND=0 RM_SINR_FRAMES=0", "RM_FILTER=grid RM_SINR_FRAMES=0"}
SWEEP_ALIASES = {"RM_SINR_GX=5": "RM_SINR_GX=5 RM_SINR_ACC=0", "RM_SINR_GX=1": "RM_SINR_GX=1 RM_SINR_ACC=0",
                 "RM_FILTER_GROUP=0": "RM_FILTER_GROUP=0 RM_NEAR_LISTS=2 RM_WG_RPT=4 RM_FILTER_TICKS_PER_WG=5"}   # (a sweep setting whose row adds what makes it engage)


def _vid(r):
    return r["env"].replace(" ", "+") or "defaults"


def _sweep_settings():
    with open(os.path.join(ROOT, "tools", "knob_sweep.sh")) as f:
        text = f.read()
    body = re.search(r"^K=\((.*?)\)\s*$", text, re.S | re.M).group(1)
    return [SWEEP_ALIASES.get(s, s) for s in re.findall(r'"([^"]*)"', body)]


def _library_knobs():
    """{knob: [(file, line number, text of the line and the two before it)]} of every read in the library"""
    found = {}
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    files = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".hpp", ".h"))]
    pkg = os.path.join(ROOT, "radio-sim_amd")
    files += [os.path.join(pkg, f) for f in sorted(os.listdir(pkg)) if f.endswith(".py")]
    pat = re.compile(r'(?:getenv\(|environ\.get\(|environ\[)\s*"(RM_[A-Z0-9_]+)"')
    for path in files:
        with open(path) as f:
            lines = f.read().split("\n")
        for i, line in enumerate(lines):
            for k in pat.findall(line):
                found.setdefault(k, []).append((os.path.basename(path), i + 1, "\n".join(lines[max(0, i - 2):i + 1])))
    return found


# ------------------------------------------------------------------------------------------------------ CPU tier
def test_every_knob_has_a_row():
    """Every RM_* knob the library reads is a row of VARIANTS or exempt; the table holds every setting of tools/knob_sweep.sh
    and the ones it lacks, and nothing else; every knob's read time is the one the source has."""
    found = _library_knobs()
    assert len(found) > 30
    in_rows = {k for r in VARIANTS for k in r["knobs"]}
    missing = sorted(set(found) - in_rows - set(EXEMPT))
    assert not missing, "knobs read by the library with no row in VARIANTS and not exempt: %s" % missing
    stale = sorted((in_rows | set(EXEMPT)) - set(found))
    assert not stale, "rows or exemptions of knobs the library no longer reads: %s" % stale
    settings = [r["env"] for r in VARIANTS]
    assert len(settings) == len(set(settings)), "a setting twice in VARIANTS"
    want = {s for s in _sweep_settings() if not any(kv.split("=")[0] in EXEMPT for kv in s.split())} | REQUIRED_EXTRA
    assert set(settings) == want, ("settings without a row: %s; rows nothing asks for: %s"
                                   % (sorted(want - set(settings)), sorted(set(settings) - want)))
    for k, sites in found.items():
        if k in EXEMPT:
            continue
        assert k in READ, "read time of %s not recorded" % k
        for f, ln, text in sites:
            once = "static const" in text
            if READ[k] == "once":
                assert once, "%s at %s:%d is not read once per process" % (k, f, ln)
            elif READ[k] == "call":
                assert not once, "%s at %s:%d is read once per process" % (k, f, ln)
    # RM_GRAPH: read when a context is made
    assert any("rm_api_context.cpp" == f for f, _, _ in found["RM_GRAPH"])
    for r in VARIANTS:
        assert r["scenarios"], r["env"]
        for sc, present, absent in r["proofs"]:
            assert sc in r["scenarios"] and (present or absent), r["env"]
        if r["covered_by"]:
            assert os.path.exists(os.path.join(ROOT, r["covered_by"])), r["covered_by"]
            with open(os.path.join(ROOT, r["covered_by"])) as f:
                assert any(k in f.read() for k in r["knobs"]), "%s does not set %s" % (r["covered_by"], r["env"])


def test_the_table_is_plain_data():
    """importing the table touches no GPU and the worker's inputs are the same in every process"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "multi"))
    import variant_worker as W
    from oracle import oracle as O
    for r in VARIANTS:
        for sc in r["scenarios"]:
            assert sc in W.SCENARIOS, sc
    a, b = W.inputs(O, "logdist_batch"), W.inputs(O, "logdist_batch")
    assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    assert [len(s) for s in a[3]] == [1, 63, 64, 65, 257]


# ------------------------------------------------------------------------------------------------------ GPU tier
_abnormal = []          # set once a child ends by a signal or a time limit: nothing more is started
_shared = {}            # the per-call child's results, by run name
_want = {}              # the oracle's side of a scenario (inputs that do not depend on the engine)


def _children():
    """[(child name, [rows], time limit in seconds)]: one child per row with a knob read once, one for all the rest"""
    out, calls = [], []
    for r in VARIANTS:
        (out.append(("v_" + _vid(r), [r])) if r["read"] == "once" else calls.append(r))
    out.insert(0, ("per_call", calls))
    return [(name, rows, 60 + sum(8 * len(r["scenarios"]) for r in rows)) for name, rows in out]


def _run_child(name, rows, limit, tmp):
    if _abnormal:
        pytest.fail("not run: an earlier variant child ended abnormally (%s)" % _abnormal[0])
    d = os.path.join(str(tmp), name)
    os.makedirs(d, exist_ok=True)
    spec = [dict(name=_vid(r), env=r["knobs"], scenarios=r["scenarios"], proof=[p[0] for p in r["proofs"]]) for r in rows]
    with open(os.path.join(d, "spec.json"), "w") as f:
        json.dump(spec, f)
    try:
        p = subprocess.run([sys.executable, WORKER, d, os.path.join(d, "spec.json")], cwd=ROOT, capture_output=True, text=True,
                           timeout=limit)
    except subprocess.TimeoutExpired:
        _abnormal.append("%s: time limit of %d s" % (name, limit))
        pytest.fail("variant child %s exceeded %d s" % (name, limit))
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _abnormal.append("%s: exit status %d" % (name, p.returncode))
    assert p.returncode == 0, "variant child %s: exit status %d\n%s\n%s" % (name, p.returncode, p.stdout[-3000:], p.stderr[-6000:])
    out = {}
    for r in rows:
        with np.load(os.path.join(d, _vid(r) + ".npz")) as z:
            res = {k: z[k] for k in z.files}
        with open(os.path.join(d, _vid(r) + ".json")) as f:
            out[_vid(r)] = (res, json.load(f))
    return out


def _same(got, want, what):
    """bit-exact links of one tick, and the offsets by packet laid out as the oracle's packet numbers give them"""
    assert int(got["count"][0]) == want.count, "%s: heard links %d (gpu) vs %d (oracle)" % (what, int(got["count"][0]), want.count)
    for f in ("pkt", "dst", "verdict"):
        np.testing.assert_array_equal(got[f], getattr(want, f), err_msg="%s %s" % (what, f))
    for f in ("rssi", "sinr"):
        np.testing.assert_array_equal(got[f].view(np.int64), np.asarray(getattr(want, f), dtype=np.float64).view(np.int64),
                                      err_msg="%s %s bits" % (what, f))
    np.testing.assert_array_equal(got["pkt_interference"], want.pkt_interference, err_msg=what + " tx failure")
    n_pk = len(got["pkt_offset"]) - 1
    off = np.concatenate([[0], np.cumsum(np.bincount(want.pkt, minlength=n_pk))])
    np.testing.assert_array_equal(got["pkt_offset"], off, err_msg=what + " pkt_offset")


def _tick(res, key):
    return {f.rsplit(".", 1)[1]: v for f, v in res.items() if f.rsplit(".", 1)[0] == key}


def check_scenario(O, sc, tag, res, what):
    """the links of one scenario's run (tag: the scenario, or its profiled rerun) against the oracle"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "multi"))
    import variant_worker as W
    if sc in ("events", "events_rings"):
        return 0    # (compared against the oracle's event replay in the child: a mismatch is the scenario's error)
    heard = 0
    if sc.startswith("gathered"):
        from radio_sim_amd import dist as D
        saved = dict(packed=res[tag + ".packed"], own=res[tag + ".own"])
        want = W.expected(O, sc, saved)
        world, slots = saved["packed"].shape[0], saved["packed"].shape[2]
        for b, w in want.items():
            parts = [_tick(res, "%s.%s.r%d" % (tag, b, r)) for r in range(world)]
            for r, p in enumerate(parts):
                assert np.all(saved["own"][p["dst"]] == r), "%s tick %s: rank %d reported another rank's receiver" % (what, b, r)
                np.testing.assert_array_equal(np.diff(p["pkt_offset"]), np.bincount(p["pkt"], minlength=world * slots),
                                              err_msg="%s tick %s rank %d pkt_offset" % (what, b, r))
                np.testing.assert_array_equal(p["pkt_interference"], parts[0]["pkt_interference"])
            merged = D.merge_shard_links([(p["pkt"], p["dst"], p["verdict"], p["rssi"], p["sinr"]) for p in parts], world * slots)
            assert len(merged[0]) == w.count, "%s tick %s: %d merged links, oracle %d" % (what, b, len(merged[0]), w.count)
            np.testing.assert_array_equal(merged[0], w.real[w.pkt], err_msg="%s tick %s pkt" % (what, b))
            for k, f in enumerate(("dst", "verdict", "rssi", "sinr"), start=1):
                np.testing.assert_array_equal(merged[k], getattr(w, f), err_msg="%s tick %s %s" % (what, b, f))
            np.testing.assert_array_equal(parts[0]["pkt_interference"][w.real], w.pkt_interference, err_msg="%s tick %s" % (what, b))
            heard += w.count
        return heard
    if sc not in _want:
        _want[sc] = W.expected(O, sc)
    for b, w in _want[sc].items():
        key = "%s.%s" % (tag, b)
        if sc == "overflow":
            dropped = int(res[key + ".dropped"][0])
            assert dropped == (1 if int(b) == 3 else 0), "%s tick %s: dropped flag %d" % (what, b, dropped)
            if dropped:
                continue
        got = _tick(res, key)
        _same(got, w, "%s tick %s" % (what, b))
        if sc in ("udgm_lone", "transmit"):
            assert int(res[key + ".rng"][0]) == w.rng_state, "%s tick %s: java.util.Random state" % (what, b)
        heard += w.count
    return heard


def _check_row(O, r, res, report):
    what = r["env"] or "defaults"
    assert not report["errors"], "%s: %s" % (what, "\n".join("%s -> %s" % kv for kv in report["errors"].items()))
    heard = 0
    for sc in r["scenarios"]:
        heard += check_scenario(O, sc, sc, res, "%s, %s" % (what, sc))
        if sc in [p[0] for p in r["proofs"]]:
            heard += check_scenario(O, sc, sc + ".prof", res, "%s, %s (profiled)" % (what, sc))
    assert heard > 0 or set(r["scenarios"]) <= {"events", "events_rings"}, what + ": nothing heard"
    for sc, present, absent in r["proofs"]:
        names = {k.split("<")[0].strip() for k in report["kernels"].get(sc, [])}
        for k in present:
            assert k in names, "%s: %s not launched by %s (launched: %s)" % (what, k, sc, sorted(names))
        for k in absent:
            assert k not in names, "%s: %s launched by %s (launched: %s)" % (what, k, sc, sorted(names))


CHILDREN = _children()


@pytest.mark.gpu
@pytest.mark.parametrize("r", VARIANTS, ids=[_vid(r) for r in VARIANTS])
def test_variant_matches_the_oracle(rsa, O, r, tmp_path_factory):
    name, rows, limit = next(c for c in CHILDREN if r in c[1])
    if name == "per_call":
        if "per_call" not in _shared:
            _shared["per_call"] = _run_child(name, rows, limit, tmp_path_factory.mktemp("variants"))
        out = _shared["per_call"]
    else:
        out = _run_child(name, rows, limit, tmp_path_factory.mktemp("variants"))
    res, report = out[_vid(r)]
    _check_row(O, r, res, report)
