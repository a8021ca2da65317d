"""The keyed-reduce (pairs) engine keeps f64 values exact: Python floats
staged by mapfn_gpu_pairs must not pass through f32 on their way in."""


def test_minmax_pairs_keep_f64(monkeypatch):
    from mapreduce_amd import run_local
    from mapreduce_amd.examples import extremes

    monkeypatch.setenv("MR_GPU_TIER", "force")
    # none of these is representable in f32
    readings = {"a": [0.1, -39.670663255201106, 44.97323567403747],
                "b": [1.0 + 2.0 ** -40, 1.0 - 2.0 ** -40]}
    extremes.init({"readings": readings})
    srv = run_local({"fns": {r: extremes for r in (
        "taskfn", "mapfn", "partitionfn", "reducefn", "combinerfn",
        "finalfn")}, "verbose": False,
        "init_args": {"readings": readings}}, nworkers=2)
    assert srv.finished and srv.stats.get("tier") == "gpu"
    assert extremes.RESULTS == {s: (min(v), max(v))
                                for s, v in readings.items()}
