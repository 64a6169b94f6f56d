"""CPU tests of bench.py's roofline bookkeeping (no GPU work: the helpers are pure arithmetic over measured numbers)."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def test_aggregate_roofline_fields_follow_survey_8d_and_no_frac_exceeds_one():
    D, nseg, f = 256, 1000, 10
    ids = torch.randint(0, 50, (nseg * f,))  # heavy reuse: 50 distinct rows
    r = bench.roofline_aggregate("MaxAggregator", D, nseg, nseg * f, avg_ms=1e-3, launches=20, ids_last=ids, workload="none",
                                 B0=1, offline_ok=False)
    assert r["algorithmic_bytes_per_launch"] == nseg * f * (4 * D + 12) + nseg * (4 * D + 4)
    assert r["distinct_rows_last_launch"] == int(torch.unique(ids).numel())
    assert r["compulsory_bytes_per_launch"] == r["distinct_rows_last_launch"] * 4 * D + nseg * f * 12 + nseg * (4 * D + 4)
    # the cache-assisted algorithmic rate has its own name; `achieved` is a rate of bytes that crossed the memory
    # system, so that achieved / peak == frac <= 1 (no field reads as bandwidth above peak)
    assert r["algorithmic_gbs"] == r["algorithmic_bytes_per_launch"] / 1e-6 / 1e9
    assert r["algorithmic_over_peak"] > 1 and r["cache_assisted"] is True
    assert r["achieved"] == r["compulsory_bytes_per_launch"] / 1e-6 / 1e9 and r["achieved"] <= r["peak"]
    assert abs(r["achieved"] / r["peak"] - r["frac"]) < 1e-12
    for k, v in r.items():
        if k.startswith("frac") and isinstance(v, float):
            assert 0 <= v <= 1, (k, v)


def test_sampler_roofline_bytes():
    r = bench.roofline_sampler("EdgeWeightSampler", 10, rows=1000, slots=10000, avg_ms=0.01, launches=3, workload="none", B0=1)
    assert r["algorithmic_bytes_per_launch"] == 10000 * 40 + 1000 * 24  # 32 B/slot + 8 B alias + 24 B/row
    r = bench.roofline_sampler("TopkSampler", 10, rows=1000, slots=10000, avg_ms=0.01, launches=3, workload="none", B0=1)
    assert r["algorithmic_bytes_per_launch"] == 10000 * 32 + 1000 * 24
    assert r["draws_per_s"] == 10000 / 1e-5


def test_committed_offline_traffic_is_labelled_and_bounded():
    ids = torch.arange(16_384_000 // 64)
    r = bench.roofline_aggregate("MaxAggregator", 256, 1_638_400, 16_384_000, avg_ms=2.15, launches=20, ids_last=ids,
                                 workload="c3", B0=65536)
    assert r["traffic"] and "OFFLINE" in r["traffic_source"] and 0 < r["frac_traffic_offline"] <= 1


def _canned(name):
    import json
    return json.load(open(os.path.join(ROOT, "profiles", "r03", name)))


def test_headline_line_stays_under_the_drivers_tail():
    """the driver keeps ~9 KB of stdout tail; round 3's 25 KB line was cut and never parsed.  The line built
    from that very record must fit 4 KB and still carry the contract's keys, `roofline` and `cpu_baseline`."""
    import json
    res = _canned("bench_c3_n1_final.json")
    assert len(json.dumps(res)) > 20000  # the record that broke the parser
    line = bench.compact_line(res, "bench_detail.json")
    assert len(line) <= bench.LINE_LIMIT < 6000 and "\n" not in line
    got = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in got, k
    assert got["value"] == pytest.approx(res["value"], rel=1e-6) and got["ms_per_step"] == pytest.approx(res["ms_per_step"], rel=1e-6)
    assert got["config"]["workload"].startswith("c3") and "model" not in got["config"]
    r = got["roofline"]
    for k in ("kernel", "bound", "peak", "unit", "achieved", "frac", "frac_basis", "algorithmic_over_peak", "frac_compulsory", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and 0 < r["frac"] <= 1 and len(r["frac_basis"]) <= 140 and not r["frac_basis"].endswith(("(", ";", ","))
    c = got["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample", "threads", "nproc", "thread_sweep"):
        assert k in c, k
    assert got["verified_vs_oracle"] is True
    oc = got["other_configs"]
    assert set(oc) == {"c2", "c5", "c4", "c3-degree-seeds"}
    for rec in oc.values():
        assert set(rec) <= {"ms_per_step", "value", "bound", "frac", "frac_basis", "traffic", "verified", "error"}
    assert got["detail"] == "bench_detail.json"


def test_headline_line_carries_the_eight_ranks_on_one_gpu_leg():
    """Round 6: the N = 1 run also times eight thread-ranks sharing the GPU (bench.edge_cut_p8_one_gpu); its two numbers and
    its verification flag ride in the line, an error record does not."""
    import json
    res = _canned("bench_c3_n1_final.json")
    res["edge_cut_p8_one_gpu"] = {"ranks": 8, "mode": "all", "ms_per_step_all_ranks": 24.54321, "ms_per_rank_step": 3.0679,
                                  "answers_equal_unpartitioned": True, "note": "x" * 300}
    got = json.loads(bench.compact_line(res, "bench_detail.json"))
    assert got["edge_cut_p8_one_gpu"] == {"ms_per_step_all_ranks": 24.5432, "ms_per_rank_step": 3.0679, "verified": True}
    res["edge_cut_p8_one_gpu"] = {"error": "TimeoutExpired"}
    line = bench.compact_line(res, "bench_detail.json")
    assert "edge_cut_p8_one_gpu" not in json.loads(line) and len(line) <= bench.LINE_LIMIT


def test_headline_line_trims_optional_blocks_before_it_would_outgrow_the_limit():
    import json
    res = _canned("bench_c3_n1_final.json")
    res["other_configs"] = {"cfg%d" % i: dict(res["other_configs"]["c2"]) for i in range(60)}  # absurdly many
    line = bench.compact_line(res, "bench_detail.json")
    got = json.loads(line)
    assert len(line) <= bench.LINE_LIMIT and "other_configs" in got["trimmed"]
    assert got["roofline"]["frac"] > 0 and got["cpu_baseline"]["value"] > 0  # the judged blocks are never dropped


def test_multi_gpu_line_is_compact_too():
    import json
    res = _canned("bench_world1_rccl_ledger.json")
    line = bench.compact_line(res, "bench_detail.json")
    got = json.loads(line)
    assert len(line) <= bench.LINE_LIMIT
    assert set(got["placements"]) >= {"features_sharded", "edge_cut_pure"}
    for leg in got["placements"].values():
        assert set(leg) <= {"ms_per_step", "value"}
    assert got["verified_sharded_equals_unpartitioned"] is True and "placement" in got["config"]["workload"]
    # the N > 1 line carries `roofline` (quoted on the 3-source reduce the partitioned step runs), parses
    # under 4 KB with nothing trimmed, and every placement leg the run timed is in it
    assert "trimmed" not in got
    r = got["roofline"]
    assert "3 row sources" in r["kernel"] and r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert 0 < r["frac"] <= 1 and r["avg_launch_ms"] > 0 and r["algorithmic_bytes_per_launch"] == 18658099200
    assert set(got["placements"]) == {"features_sharded_serial", "features_replicated", "features_sharded", "features_sharded_speculated",
                                      "edge_cut_pure", "edge_cut_pure_speculated", "edge_cut_pure_design_r"}
    assert set(got["verified_legs"]) >= {"features_sharded", "features_sharded_speculated", "edge_cut_pure", "edge_cut_pure_design_r"}
    assert all(got["verified_legs"].values())
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "cpu_baseline"):
        assert k in got, k


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libglref.so")), reason="oracle/_ref not built")
def test_cpu_baseline_runs_both_storage_modes_at_every_thread_count():
    """the reference's CPU path on the whole graph, StorageMode 2 and 3, T = 1 / .. / nproc -> six numbers,
    `value` = the best of them (here on the tiny workload with two thread counts)."""
    import argparse
    V, E = bench.WORKLOADS["tiny"][:2]
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, V, (E,), generator=g)
    dst = torch.randint(0, V, (E,), generator=g)
    w = torch.rand(E, generator=g) + 0.01
    args = argparse.Namespace(workload="tiny", cpu_storage_modes="3,2", cpu_time_budget=0.2, cpu_seeds_per_request=16,
                              cpu_thread_sweep="1,2", cpu_edge_limit=0, cpu_wall_limit=300.0)
    r = bench.cpu_baseline(bench.WORKLOADS["tiny"], src, dst, w, args, torch.unique(src).numpy())
    assert r["kind"] == "reference" and r["errors"] is None, r
    assert set(r["modes"]) == {"2", "3"} and all(set(v) == {"1", "2"} for v in r["modes"].values())
    six = [v for m in r["modes"].values() for v in m.values()]
    assert r["value"] == max(six) > 0 and r["edges_built"] == E and r["feature_rows"] == V
    assert r["cores"] in (1, 2) and r["storage_mode"] in (2, 3)
    c = bench.compact_cpu(r)
    assert set(c["modes"]) == {"2", "3"} and len(c["sample"]) <= 160 and c["storage_mode"] == r["storage_mode"]


def test_bench_refuses_more_gpus_than_are_visible_with_one_json_line():
    """`python bench.py --gpus N` without a launcher re-executes itself under torch.distributed.run -- unless the box
    has fewer devices than asked for: then ONE JSON error line and a non-zero exit, never a 1-GPU number under an N-GPU
    label.  Here (any box with fewer than 64 GPUs, this CPU container included)."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--workload", "tiny", "--steps", "2"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 2, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["value"] is None and "--gpus 64" in res["error"] and res["n_gpus"] < 64 and res["metric"]


def _args(**kw):
    import argparse
    base = dict(workload="c3", batch=65536, cpu_baseline="on", host_boundary="on", roofline_probes="on", verify_oracle="on",
                request_shape_legs="on", small_batches="on", edge_cut_probe="on", other_configs="c2,c5")
    base.update(kw)
    return argparse.Namespace(**base)


def test_side_measurements_are_n1_only():
    """with more than one rank none of the N = 1 side measurements (CPU baseline, host boundary,
    other configs, probes, small batches, the world-1 edge-cut probe) runs, so an 8-rank job fits its lease."""
    one = bench.n1_extras(_args(), world=1, sharded=False)
    assert all(one.values()), one
    for world, sharded in ((2, True), (8, True), (1, True)):
        many = bench.n1_extras(_args(), world=world, sharded=sharded)
        assert not any(many.values()), (world, sharded, many)
    # the extras tied to the headline workload do not run for the others, nor at other batch sizes
    c2 = bench.n1_extras(_args(workload="c2"), world=1, sharded=False)
    assert c2["cpu_baseline"] and not c2["other_configs"] and not c2["edge_cut_probe"]
    small = bench.n1_extras(_args(batch=1024), world=1, sharded=False)
    assert not small["small_batches"] and not small["other_configs"]
    off = bench.n1_extras(_args(cpu_baseline="off", other_configs=""), world=1, sharded=False)
    assert not off["cpu_baseline"] and not off["other_configs"]


def test_plain_run_times_the_headline_alone_and_full_runs_every_side_measurement():
    """A plain `bench.py --gpus 1` run does what its headline needs: the request-shape legs (the headline quotes the slowest
    of them) and nothing else; --full turns every side measurement on, and an option named on the command line wins."""
    plain = bench.n1_extras(bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "3"]), world=1, sharded=False)
    assert plain.pop("request_shape_legs") and not any(plain.values()), plain
    full_args = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "3", "--full"])
    assert all(bench.n1_extras(full_args, world=1, sharded=False).values())
    assert full_args.other_configs == "c2,c5,c4,c3-degree-seeds"
    one = bench.n1_extras(bench.parse_args(["--roofline-probes", "on"]), world=1, sharded=False)
    assert one["roofline_probes"] and not one["cpu_baseline"] and not one["other_configs"]
    less = bench.n1_extras(bench.parse_args(["--full", "--cpu-baseline", "off", "--other-configs", ""]), world=1, sharded=False)
    assert not less["cpu_baseline"] and not less["other_configs"] and less["verify_oracle"]


def test_compact_line_keeps_whole_clauses_and_the_request_shape_legs():
    res = {"metric": "m", "value": 1.0, "unit": "edges/s", "n_gpus": 1, "steps": 2, "warmup": 1, "ms_per_step": 2.3,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "c3: x", "seeds": "uniform over the vertices that have out-edges (a training set has "
                                                    "neighbours; harder than SURVEY 8(d)'s), fresh batch every step",
                      "segment_ids": "implied by the dense sampler response (segment i = row i's neighbours)"},
           "roofline": {"bound": "hbm", "peak": 8000.0, "unit": "GB/s", "achieved": 5250.0, "frac": 0.656,
                        "algorithmic_gbs": 9985.0, "memory_side_gbs": 7400.0, "traffic": 1.38e10, "kernel": "k",
                        "achieved_basis": "cache-free leg: algorithmic bytes (== memory-side traffic there) / its average launch time",
                        "frac_basis": "cache-free leg of this run: the same kernel on the same request shape with ids uniform "
                                      "over the table (algorithmic bytes == memory-side traffic; more) / 8 TB/s"},
           "request_shapes": {"headline_shape_ms": 2.30, "with_segment_ids_ms": 2.31, "seeds_uniform_over_V_ms": 1.9,
                              "headline_is": "headline_shape"}}
    import json
    line = bench.compact_line(res)
    got = json.loads(line)
    assert got["config"]["seeds"] == "uniform over the vertices that have out-edges"
    assert got["config"]["segment_ids"] == "implied by the dense sampler response"
    assert got["roofline"]["frac_basis"].endswith("ids uniform over the table")  # a whole clause, not cut mid-word
    assert got["roofline"]["achieved"] <= got["roofline"]["peak"] and got["roofline"]["algorithmic_gbs"] == 9985.0
    assert got["request_shapes"]["with_segment_ids_ms"] == 2.31 and got["request_shapes"]["headline_is"] == "headline_shape"


def test_dump_outputs_keeps_to_its_budget_and_is_deterministic(tmp_path, monkeypatch):
    """--dump-outputs: every array as <name>.npy in float32 / float64, within DUMP_LIMIT bytes; an output too large is cut
    to the same seeded rows on every call, named in rows_<group>.npy, and the values are the rows they claim to be."""
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_LIMIT", 1 << 20)
    g = torch.Generator().manual_seed(0)
    nb1 = torch.randint(0, 1 << 40, (64, 5), generator=g)
    emb1 = torch.randn(64, 16, generator=g)
    nb2 = torch.randint(0, 1 << 40, (320, 3), generator=g)
    emb2 = torch.randn(320, 1024, generator=g)  # 1.3 MB as float32: more than the whole budget
    cnt1, cnt2 = torch.randint(0, 6, (64,), generator=g, dtype=torch.int32), torch.randint(0, 4, (320,), generator=g, dtype=torch.int32)
    groups = bench.hop_outputs(nb1, nb1 + 1, emb1, cnt1, nb2, nb2 - 1, emb2, cnt2)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        bench.dump_outputs(str(d), groups)
    files = sorted(p.name for p in dirs[0].iterdir())
    assert files == sorted(["rows_hop1.npy", "rows_hop2.npy"] + [k + ".npy" for _, a in groups for k in a])
    assert sum((dirs[0] / f).stat().st_size for f in files) <= (1 << 20) + 4096 * len(files)  # + the .npy headers
    for f in files:
        x, y = np.load(dirs[0] / f), np.load(dirs[1] / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    r1, r2 = np.load(dirs[0] / "rows_hop1.npy"), np.load(dirs[0] / "rows_hop2.npy")
    assert np.array_equal(r1, np.arange(64)) and 0 < r2.shape[0] < 320  # the small group whole, the large one sampled
    rows = r2.astype(np.int64)
    assert np.array_equal(np.load(dirs[0] / "hop2_aggregate.npy"), emb2.numpy()[rows])
    assert np.array_equal(np.load(dirs[0] / "hop2_neighbors.npy"), nb2.numpy()[rows].astype(np.float64))
    assert np.array_equal(np.load(dirs[0] / "hop1_counts.npy"), cnt1.numpy().astype(np.float64))
