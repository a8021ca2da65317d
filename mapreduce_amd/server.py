"""Server (driver/orchestrator).

Parity with mapreduce/server.lua: configures a task from user function
modules, inserts map jobs, polls until all maps are WRITTEN, creates reduce
jobs from the shuffle files, polls reduces, computes per-phase statistics,
runs finalfn, supports finalfn->"loop" for iterative MapReduce, and restores
half-finished tasks on restart (loop :466-611, restore :470-504,
prepare_map :249-276, prepare_reduce :279-329, final :348-413, stats
:540-601).

Differences by design (MI355X-native):
  * control plane = TCPStore CAS (mapreduce_amd.parallel.coord), not Mongo;
  * stats are reduced in-process from the job documents instead of Mongo's
    server-side JS map-reduce (server.lua:155-183);
  * an optional heartbeat timeout requeues jobs of dead workers — a
    liveness gap in the reference.
"""

from __future__ import annotations

import re
import sys
import time
from typing import Any, Dict, List, Optional

from . import fs as fsmod
from .job import FnSet
from .parallel.coord import Coordinator, connect
from .task import Task, make_job
from .utils import (DEFAULT_HEARTBEAT_TIMEOUT, DEFAULT_SLEEP,
                    MAX_TASKFN_VALUE_SIZE, STATUS, TASK_STATUS,
                    assert_check, gettime)


class Server:
    def __init__(self, cnn_string: str = "local", db: str = "mr",
                 coord: Optional[Coordinator] = None, listen: bool = True):
        self.coord = coord or connect(cnn_string, db, listen=listen)
        self.task = Task(self.coord)
        self.params: Optional[dict] = None
        self.finished = False
        self.iteration = 1
        self._errors_drained = 0
        self.stats: Dict[str, Any] = {}
        self.poll_interval = DEFAULT_SLEEP
        self.heartbeat_timeout: Optional[float] = DEFAULT_HEARTBEAT_TIMEOUT
        self.verbose = True

    # ------------------------------------------------------------ configure
    def configure(self, params: dict) -> "Server":
        """Validate + normalize config (server.lua:419-462).

        params: fns = {taskfn, mapfn, partitionfn, reducefn[, combinerfn,
        finalfn]} (module names or objects; one object may provide all
        roles), storage = "mem|shared[:path]", result_ns, init_args.
        """
        fns = dict(params.get("fns") or {})
        for role in ("taskfn", "mapfn", "partitionfn", "reducefn"):
            if not fns.get(role):
                raise ValueError(f"needs a {role} module (server.lua:427-428)")
        fns.setdefault("combinerfn", None)
        fns.setdefault("finalfn", None)
        from .job import spec_of

        fns = {role: spec_of(m) for role, m in fns.items()}
        storage = params.get("storage") or "shared"
        self.params = {
            "fns": fns,
            "storage": storage,
            "path": params.get("path", ""),
            "result_ns": params.get("result_ns", "result"),
            "init_args": params.get("init_args"),
        }
        self.poll_interval = params.get("poll_interval", DEFAULT_SLEEP)
        # default ON: executing workers heartbeat their job docs, so a
        # requeue only fires for genuinely dead claim holders; pass
        # heartbeat_timeout=None to disable (and disable worker
        # heartbeats with it, or long jobs will be requeued)
        self.heartbeat_timeout = params.get("heartbeat_timeout",
                                            DEFAULT_HEARTBEAT_TIMEOUT)
        # no-progress watchdog: if NOTHING completes for this long while
        # jobs remain, force-fail the stuck WAITING/BROKEN ones so the
        # task terminates with a failure count instead of polling forever
        # (the reference polls forever, server.lua:515-533; progress of
        # any kind resets the clock, so slow-but-alive pools are safe)
        self.stall_timeout = params.get("stall_timeout", 600.0)
        self.verbose = params.get("verbose", True)
        self.fns = FnSet(fns, self.params["init_args"])
        # a malformed "group", "window", "asof" or "graph" family reducer
        # is refused here, not mid-task
        self.parse_group_reducer(self.fns.reducefn_gpu)
        self.parse_window_reducer(self.fns.reducefn_gpu)
        self.parse_asof_reducer(self.fns.reducefn_gpu)
        self.parse_graph_reducer(self.fns.reducefn_gpu)
        self.fs = fsmod.router(storage, self.params["path"])
        return self

    def _log(self, msg: str) -> None:
        if self.verbose:
            print(f"# {msg}", file=sys.stderr, flush=True)

    # ------------------------------------------------- GPU-tier dispatch
    # The reference routes each reduce through a fast path when the
    # reducer declares associative+commutative+idempotent
    # (job.lua:104-106, 264-274).  The MI355X analogue is framework-level:
    # when the task module also provides the GPU staging hook
    # (mapfn_gpu) and names a builtin fused reduction (reducefn_gpu),
    # the WHOLE job runs on the HIP engine under the same
    # Server.configure(...).loop() entry point; anything else falls back
    # to the host tier's general Python executor.

    GPU_REDUCERS = ("sum",)  # fused text engine (wordcount family)
    GPU_PAIR_REDUCERS = ("sum", "min", "max", "minmax")  # keyed-reduce
    # equi-join of two staged relations: reducer name -> JoinJob how
    GPU_JOIN_REDUCERS = {"join": "inner", "join_left": "left",
                         "join_semi": "semi", "join_anti": "anti"}
    # per-key order statistics: reducers over the whole value list of a key
    GPU_GROUP_REDUCERS = ("group", "median", "quantile", "topk", "bottomk",
                          "distinct")

    @classmethod
    def parse_group_reducer(cls, name):
        """reducefn_gpu of the "group" family -> (op, parameter), or None
        when the name belongs to another family.  "group", "median" and
        "distinct" take no parameter; "quantile:N/D[,N/D...]" gives a list
        of (N, D); "topk:K" and "bottomk:K" give K.  A malformed parameter
        raises ValueError naming the string."""
        if not isinstance(name, str):
            return None
        op, sep, arg = name.partition(":")
        if op not in cls.GPU_GROUP_REDUCERS:
            return None
        bad = ValueError(
            f"malformed reducefn_gpu {name!r}: expected 'group', 'median', "
            "'distinct', 'quantile:N/D[,N/D...]' with 0 <= N <= D <= 10^6 "
            "(at most 8), 'topk:K' or 'bottomk:K' with K >= 1")
        if op in ("group", "median", "distinct"):
            if sep:
                raise bad
            return op, None
        if op in ("topk", "bottomk"):
            if not (arg.isascii() and arg.isdigit() and int(arg) >= 1):
                raise bad
            return op, int(arg)
        fracs = []
        for part in arg.split(","):
            n, slash, d = part.partition("/")
            if not (slash and n.isascii() and n.isdigit() and d.isascii()
                    and d.isdigit()):
                raise bad
            fracs.append((int(n), int(d)))
        from . import ops
        if not 1 <= len(fracs) <= ops.GROUP_QMAX or any(
                not (1 <= d <= ops.GROUP_MAX_DEN and n <= d)
                for n, d in fracs):
            raise bad
        return op, fracs

    # per-key running aggregates and sessions: reducers over the ordered
    # rows of a key whose answer is as long as their input
    GPU_WINDOW_REDUCERS = {"cumsum": "sum", "cummin": "min", "cummax": "max",
                           "sessions": None}

    @classmethod
    def parse_window_reducer(cls, name):
        """reducefn_gpu of the "window" family -> (op, parameter), or None
        when the name belongs to another family.  "cumsum", "cummin" and
        "cummax" take no parameter; "sessions:GAP" gives GAP, a decimal
        integer with 0 <= GAP < 2^63; "rolling:OP:PRE[,fol=N][,rows]" gives
        {"op", "preceding", "following", "unit"} (_parse_rolling).  A
        malformed name raises ValueError naming the string."""
        if not isinstance(name, str):
            return None
        op, sep, arg = name.partition(":")
        if op == "rolling":
            return op, cls._parse_rolling(name, arg)
        if op not in cls.GPU_WINDOW_REDUCERS:
            return None
        bad = ValueError(
            f"malformed reducefn_gpu {name!r}: expected 'cumsum', 'cummin', "
            "'cummax' or 'sessions:GAP' with a decimal 0 <= GAP < 2^63")
        if op != "sessions":
            if sep:
                raise bad
            return op, None
        if not (arg.isascii() and arg.isdigit() and int(arg) < 2 ** 63):
            raise bad
        return op, int(arg)

    GPU_ROLLING_OPS = ("sum", "min", "max", "count", "mean")

    @classmethod
    def _parse_rolling(cls, name, arg):
        """The part of "rolling:OP:PRE[,fol=N][,rows]" behind "rolling:" ->
        {"op", "preceding", "following", "unit"}.  OP is one of
        GPU_ROLLING_OPS; PRE and N are decimal integers, below 2^63 for a
        range frame and below 2^31 with "rows"; each option appears at most
        once."""
        bad = ValueError(
            f"malformed reducefn_gpu {name!r}: expected "
            "'rolling:OP:PRE[,fol=N][,rows]' with OP one of "
            f"{'/'.join(cls.GPU_ROLLING_OPS)} and decimal PRE and N, below "
            "2^63 (2^31 with 'rows')")

        def num(txt):
            if not (txt.isascii() and txt.isdigit()):
                raise bad
            return int(txt)

        agg, sep, rest = arg.partition(":")
        if agg not in cls.GPU_ROLLING_OPS or not sep:
            raise bad
        pre, *opts = rest.split(",")
        out = {"op": agg, "preceding": num(pre), "following": None,
               "unit": None}
        for o in opts:
            if o == "rows" and out["unit"] is None:
                out["unit"] = "rows"
            elif o.startswith("fol=") and out["following"] is None:
                out["following"] = num(o[4:])
            else:
                raise bad
        out["following"] = out["following"] or 0
        out["unit"] = out["unit"] or "range"
        limit = 2 ** 31 if out["unit"] == "rows" else 2 ** 63
        if out["preceding"] >= limit or out["following"] >= limit:
            raise bad
        return out

    # as-of join of two staged, time-ordered relations
    GPU_ASOF_REDUCER = "join_asof"

    @classmethod
    def parse_asof_reducer(cls, name):
        """reducefn_gpu of the "asof" family -> {"direction", "allow_exact",
        "how", "tolerance"}, or None when the name belongs to another
        family.  "join_asof" alone is backward, exact matches allowed, every
        left row kept, no tolerance; "join_asof:OPT[,OPT...]" takes at most
        one of backward / forward / nearest, "strict" (no exact matches),
        "inner" (matched rows only) and "tol=N", a decimal integer with
        0 <= N < 2^63.  A malformed name raises ValueError naming the
        string."""
        if not isinstance(name, str):
            return None
        op, sep, arg = name.partition(":")
        if op != cls.GPU_ASOF_REDUCER:
            return None
        bad = ValueError(
            f"malformed reducefn_gpu {name!r}: expected 'join_asof' or "
            "'join_asof:OPT[,OPT...]' with each option once: one of "
            "'backward', 'forward', 'nearest'; 'strict'; 'inner'; 'tol=N' "
            "with a decimal 0 <= N < 2^63")
        opts = {"direction": None, "allow_exact": True, "how": "left",
                "tolerance": None}
        if not sep:
            opts["direction"] = "backward"
            return opts
        seen = set()
        for part in arg.split(","):
            if part in ("backward", "forward", "nearest"):
                what = "direction"
                opts["direction"] = part
            elif part == "strict":
                what = "strict"
                opts["allow_exact"] = False
            elif part == "inner":
                what = "inner"
                opts["how"] = "inner"
            elif part.startswith("tol="):
                n = part[4:]
                if not (n.isascii() and n.isdigit() and int(n) < 2 ** 63):
                    raise bad
                what = "tol"
                opts["tolerance"] = int(n)
            else:
                raise bad
            if what in seen:
                raise bad
            seen.add(what)
        if opts["direction"] is None:
            opts["direction"] = "backward"
        return opts

    # iterative jobs over a resident graph: every key reduces a value
    # gathered from other keys over its edge list
    GPU_GRAPH_REDUCERS = ("pagerank", "components")

    @classmethod
    def parse_graph_reducer(cls, name):
        """reducefn_gpu of the "graph" family -> {"algo": "pagerank",
        "damping", "iters", "tol"} or {"algo": "components"}, or None when
        the name belongs to another family.  "pagerank" alone is d=0.85,
        iters=100, tol=0; "pagerank:OPT[,OPT...]" takes each of "d=D" (a
        decimal in [0, 1]), "iters=N" (a decimal integer >= 1) and "tol=T"
        (a finite decimal >= 0) at most once; "components" takes no option.
        A malformed name raises ValueError naming the string."""
        if not isinstance(name, str):
            return None
        op, sep, arg = name.partition(":")
        if op not in cls.GPU_GRAPH_REDUCERS:
            return None
        bad = ValueError(
            f"malformed reducefn_gpu {name!r}: expected 'components' or "
            "'pagerank[:d=D][,iters=N][,tol=T]' with each option once, a "
            "decimal 0 <= D <= 1, a decimal integer N >= 1 and a finite "
            "decimal T >= 0")
        if op == "components":
            if sep:
                raise bad
            return {"algo": op}
        opts = {"algo": op, "damping": 0.85, "iters": 100, "tol": 0.0}
        if not sep:
            return opts
        import math
        import re
        dec = re.compile(r"(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?")
        seen = set()
        for part in arg.split(","):
            what, eq, txt = part.partition("=")
            if not eq or what in seen or not txt.isascii():
                raise bad
            seen.add(what)
            if what == "iters":
                if not txt.isdigit() or int(txt) < 1:
                    raise bad
                opts["iters"] = int(txt)
            elif what in ("d", "tol"):
                if not dec.fullmatch(txt) or not math.isfinite(float(txt)):
                    raise bad
                x = float(txt)
                if what == "d" and x > 1.0:
                    raise bad
                opts["damping" if what == "d" else "tol"] = x
            else:
                raise bad
        return opts

    def _gpu_engine_kind(self) -> Optional[str]:
        """Which GPU engine family this task routes to, or None.

        Ten families (one worked example each; README table):
          "bytes"   mapfn_gpu + reducefn_gpu="sum" — fused tokenize/
                    combine wordcount engine (examples/wordcount)
          "pairs"   mapfn_gpu_pairs + sum/min/max/minmax — keyed
                    segmented reduce (examples/extremes)
          "sort"    mapfn_gpu_pairs + "sort" — distributed radix sort
                    (examples/terasort_task)
          "index"   mapfn_gpu + "index" — inverted index
                    (examples/inverted_index)
          "gradsum" mapfn_gpu_grads + "gradsum" — bucketed RCCL
                    gradient allreduce (examples/train_digits, kmeans)
          "join"    mapfn_gpu_pairs + join/join_left/join_semi/join_anti
                    — equi-join of two relations (examples/join_tables)
          "group"   mapfn_gpu_pairs + group/median/quantile:N/D,.../
                    topk:K/bottomk:K/distinct — per-key order statistics
                    over the whole value list (examples/percentiles)
          "window"  mapfn_gpu_pairs + cumsum/cummin/cummax/sessions:GAP/
                    rolling:OP:PRE[,fol=N][,rows] — per-key running and
                    rolling aggregates and sessions over the ordered rows
                    (examples/sessions, examples/rolling_spend)
          "asof"    mapfn_gpu_pairs + join_asof[:backward|forward|nearest,
                    strict,inner,tol=N] — as-of join of two time-ordered
                    relations (examples/asof_quotes)
          "graph"   mapfn_gpu_pairs + pagerank[:d=D][,iters=N][,tol=T]/
                    components — iterative jobs over a graph kept resident
                    on the device (examples/pagerank)

        MR_GPU_TIER=off forces host tier; =force routes the GPU data
        path onto the CPU-ops engine (testing without a GPU)."""
        import os
        mode = os.environ.get("MR_GPU_TIER", "auto")
        if mode == "off":
            return None
        fns = self.fns
        kind = None
        if (callable(fns.mapfn_gpu)
                and fns.reducefn_gpu in self.GPU_REDUCERS
                and fns.associative and fns.commutative):
            kind = "bytes"
        elif (callable(fns.mapfn_gpu_grads)
              and fns.reducefn_gpu == "gradsum"
              and fns.associative and fns.commutative):
            # iterative gradient training (the APRIL-ANN shape): map
            # jobs produce named gradient tensors, the reduce is one
            # bucketed RCCL allreduce (K6)
            kind = "gradsum"
        elif (callable(fns.mapfn_gpu)
              and fns.reducefn_gpu == "index"):
            # inverted index: the "reduce" is a group-by (no combining
            # arithmetic), exact by construction — no property flags
            # needed; mapfn_gpu stages raw split bytes like "bytes"
            kind = "index"
        elif (callable(fns.mapfn_gpu_pairs)
              and fns.reducefn_gpu == "sort"):
            # distributed sort: no reduction at all (reducefn is the
            # identity), so no property flags are required — the output
            # contract is global key order (TeraSort family)
            kind = "sort"
        elif (callable(fns.mapfn_gpu_pairs)
              and fns.reducefn_gpu in self.GPU_JOIN_REDUCERS):
            # equi-join: the "reduce" pairs the two relations' rows of a
            # key, exact by construction — no property flags needed
            kind = "join"
        elif (callable(fns.mapfn_gpu_pairs)
              and self.parse_group_reducer(fns.reducefn_gpu) is not None):
            # reducers over the whole value list of a key: not
            # associative, so there are no property flags to require
            kind = "group"
        elif (callable(fns.mapfn_gpu_pairs)
              and self.parse_window_reducer(fns.reducefn_gpu) is not None):
            # running aggregates and sessions depend on the order of a
            # key's rows: not associative either, no property flags
            kind = "window"
        elif (callable(fns.mapfn_gpu_pairs)
              and self.parse_asof_reducer(fns.reducefn_gpu) is not None):
            # the as-of join walks the two relations' rows of a key in
            # time order: exact by construction, no property flags
            kind = "asof"
        elif (callable(fns.mapfn_gpu_pairs)
              and self.parse_graph_reducer(fns.reducefn_gpu) is not None):
            # the iteration is defined by the engine, not by a reducer
            # whose properties could be declared: no property flags
            kind = "graph"
        elif (callable(fns.mapfn_gpu_pairs)
              and fns.reducefn_gpu in self.GPU_PAIR_REDUCERS
              and fns.associative and fns.commutative
              # min/max re-apply at both reduce levels; the reference's
              # own precondition for that is the idempotent flag
              and (fns.reducefn_gpu == "sum" or fns.idempotent)):
            kind = "pairs"
        if kind is None:
            return None
        if mode == "force":
            return kind
        import torch
        return kind if torch.cuda.is_available() else None

    def gpu_tier_eligible(self) -> bool:
        return self._gpu_engine_kind() is not None

    def _collect_taskfn_jobs(self) -> List[tuple]:
        """Run taskfn(emit) with the reference's validation (dup keys,
        16 KB values — server.lua:258-267) and return [(key, value)]."""
        import pickle
        jobs: List[tuple] = []
        seen = set()

        def emit(key, value):
            k = str(key)
            if k in seen:
                raise ValueError(f"duplicate taskfn key {key!r} "
                                 "(server.lua:258-261)")
            seen.add(k)
            assert_check(value)
            if len(pickle.dumps(value)) > MAX_TASKFN_VALUE_SIZE:
                raise ValueError(
                    f"taskfn value for key {key!r} exceeds "
                    f"{MAX_TASKFN_VALUE_SIZE} bytes (server.lua:262-267)")
            jobs.append((k, value))

        self.fns.taskfn(emit)
        return jobs

    def _gpu_finalize_round(self, pairs, rank: int, world: int,
                            sort_key=None):
        """Shared tail of every GPU engine round: gather the per-rank
        result pairs to rank 0 (C8), order them (sort_key=None keeps
        the gathered rank-major order — the sort engine's global
        order), run finalfn there, and broadcast the reply so every
        rank agrees on loop/finish."""
        if world > 1:
            import torch.distributed as td
            gathered = [None] * world if rank == 0 else None
            td.gather_object(pairs, gathered, dst=0)
            if rank == 0:
                pairs = [p for g in gathered for p in g]
        if sort_key is not None and rank == 0:
            pairs.sort(key=sort_key)
        reply = True
        if rank == 0 and self.fns.finalfn is not None:
            reply = self.fns.finalfn(iter(pairs))
        if world > 1:
            import torch.distributed as td
            box = [reply]
            td.broadcast_object_list(box, src=0)
            reply = box[0]
        return reply

    def _loop_gpu(self) -> None:
        """Drive the task on the GPU engine: stage each rank's map-job
        bytes into device memory, run the fused
        tokenize/combine/shuffle/reduce under control-plane job tracking
        (GpuClusterRunner), gather per-rank results to rank 0, and run
        finalfn there — same iterate-on-"loop" semantics as the host
        tier (server.lua:389-399).

        Multi-GPU: launch the same server program under torchrun (one
        rank per GPU); every rank calls loop(), map jobs are assigned
        round-robin by rank, and rank 0 owns finalfn — its reply is
        broadcast so all ranks agree on iteration/termination."""
        import numpy as np
        import torch

        from .gpu import dist as dx
        from .gpu.runner import GpuClusterRunner
        from .gpu.wordcount import WordCountJob

        t_start = gettime()
        rank, world = dx.world_info()
        if torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        else:
            device = torch.device("cpu")
        engine = None
        runner = None
        staged = None  # (jobs_signature, text, splits) — iteration reuse
        while not self.finished:
            jobs = self._collect_taskfn_jobs()
            mine = [kv for i, kv in enumerate(jobs) if i % world == rank]
            sig = [k for k, _ in mine]
            if staged is None or staged[0] != sig:
                # stage this rank's splits once per distinct job list —
                # iterative runs reuse the HBM-resident corpus, the
                # engine-side analogue of the reference's map-job
                # affinity cache (task.lua:279-293)
                blobs = [self.fns.mapfn_gpu(k, v) for k, v in mine]
                splits = []
                off = 0
                for b in blobs:
                    splits.append((off, off + len(b)))
                    off += len(b) + 1  # '\n' joint keeps splits
                    #                    whitespace-aligned
                joined = b"\n".join(bytes(b) for b in blobs)
                text = torch.from_numpy(
                    np.frombuffer(joined, dtype=np.uint8).copy()).to(device)
                staged = (sig, text, splits)
            _, text, splits = staged
            if engine is None:
                engine = WordCountJob(device, timing=True)
                runner = GpuClusterRunner(engine, coord=self.coord,
                                          ns_suffix="_gpu")
            runner.iteration = self.iteration
            result = runner.run(text, splits)
            self.iteration = runner.task.iteration() or self.iteration
            # C7/C8: per-rank sorted results -> host pairs (lex order =
            # the reference's sorted-result guarantee, server.lua:360-385)
            pairs = [(k.decode("utf-8", "surrogateescape"), [v])
                     for k, v in result.to_host(order="lex")]
            reply = self._gpu_finalize_round(pairs, rank, world,
                                             sort_key=lambda kv: kv[0])
            if reply == "loop":
                self.iteration += 1
                self._log(f"iterative loop -> iteration {self.iteration}")
            else:
                self.finished = True
        # stats in the host tier's shape (server.lua:557-602), from
        # HIP-event phase times
        pm = dict(engine.last_phase_ms or {})
        self.stats.update({
            "tier": "gpu",
            "map_failed": 0, "reduce_failed": 0,
            "map": {"sum_cpu_time": 0.0,
                    "sum_real_time": sum(v for k, v in pm.items()
                                         if k.startswith("map")) / 1e3,
                    "cluster_time": sum(v for k, v in pm.items()
                                        if k.startswith("map")) / 1e3,
                    "jobs": len(splits)},
            "reduce": {"sum_cpu_time": 0.0,
                       "sum_real_time": pm.get("shuffle_reduce", 0.0) / 1e3,
                       "cluster_time": pm.get("shuffle_reduce", 0.0) / 1e3,
                       "jobs": world},
            "total_time": gettime() - t_start,
            "phase_ms": pm,
        })
        self.print_stats()

    def _loop_gpu_pairs(self) -> None:
        """Keyed-reduce GPU engine: the task's emitted (key, value)
        pairs are staged as device tensor columns (mapfn_gpu_pairs) and
        reduced with the segmented sum/min/max HIP kernels
        (KeyedReduceJob: local combine -> mulhi-partitioned all-to-all
        of uniques -> final reduce — the two-level split of
        job.lua:198-201/:264-284).  "minmax" runs the min and max
        reductions over the same columns, yielding (lo, hi) envelope
        values (the extremes example's reducer).

        Contract: keys must be int64-representable; the value dtype
        must be uniform across ranks (float -> f64, int -> i64)."""
        import torch

        from .gpu import dist as dx
        from .gpu.keyed_reduce import KeyedReduceJob

        t_start = gettime()
        rank, world = dx.world_info()
        device = (torch.device("cuda", torch.cuda.current_device())
                  if torch.cuda.is_available() else torch.device("cpu"))
        op = self.fns.reducefn_gpu
        decode = self.fns.gpu_key_decode or (lambda k: k)
        gtask = Task(self.coord, key="task_gpu")
        staged = None  # (job signature, keys, vals) — iteration reuse
        while not self.finished:
            if rank == 0:
                gtask.create_collection(TASK_STATUS.WAIT, {
                    "fns": {"engine": f"keyed_reduce:{op}"},
                    "storage": "hbm", "result_ns": "result",
                }, self.iteration)
            jobs = self._collect_taskfn_jobs()
            mine = [kv for i, kv in enumerate(jobs) if i % world == rank]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.MAP)
            sig = [k for k, _ in mine]
            if staged is None or staged[0] != sig:
                # stage once per distinct job list; iterative runs reuse
                # the HBM-resident columns (the affinity-cache analogue,
                # task.lua:279-293 — same as the bytes engine)
                kcols, vcols = [], []
                for k, v in mine:
                    ks, vs = self.fns.mapfn_gpu_pairs(k, v)
                    kcols.append(torch.as_tensor(ks, dtype=torch.int64))
                    # floats stage as f64 from the start: as_tensor's
                    # default (f32) would round them before the widening
                    vt = torch.as_tensor(vs)
                    vcols.append(torch.as_tensor(vs, dtype=torch.float64)
                                 if vt.is_floating_point()
                                 else vt.to(torch.int64))
                if kcols:
                    keys = torch.cat(kcols).to(device)
                    vals = torch.cat(vcols).to(device)
                else:
                    keys = torch.empty(0, dtype=torch.int64, device=device)
                    vals = torch.empty(0, dtype=torch.float64,
                                       device=device)
                staged = (sig, keys, vals)
            _, keys, vals = staged
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.REDUCE)
            if op == "minmax":
                uk, lo = KeyedReduceJob(device, op="min").run(keys, vals)
                _, hi = KeyedReduceJob(device, op="max").run(keys, vals)
                pairs = [(decode(int(k)), [(l, h)]) for k, l, h in
                         zip(uk.cpu().tolist(), lo.cpu().tolist(),
                             hi.cpu().tolist())]
            else:
                uk, uv = KeyedReduceJob(device, op=op).run(keys, vals)
                pairs = [(decode(int(k)), [v]) for k, v in
                         zip(uk.cpu().tolist(), uv.cpu().tolist())]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.FINISHED)
            reply = self._gpu_finalize_round(
                pairs, rank, world, sort_key=lambda kv: str(kv[0]))
            if reply == "loop":
                self.iteration += 1
                self._log(f"iterative loop -> iteration {self.iteration}")
            else:
                self.finished = True
        self.stats.update({
            "tier": "gpu", "engine": f"keyed_reduce:{op}",
            "map_failed": 0, "reduce_failed": 0,
            "total_time": gettime() - t_start,
        })
        self.print_stats()

    def _loop_gpu_grads(self) -> None:
        """Gradient-training GPU engine (the APRIL-ANN iterative shape,
        SURVEY.md §3.5): each map job computes named gradient tensors
        (mapfn_gpu_grads), the reduce is a local accumulate + ONE
        bucketed RCCL allreduce over xGMI (K6, gpu/gradsum.py) — the
        reference's GridFS model exchange + Mongo gradient shuffle
        collapse into collectives.

        DDP-style replica semantics: the allreduce leaves the IDENTICAL
        summed gradients on every rank, and finalfn runs on EVERY rank
        (deterministic update keeps the model replicas in sync — no
        model broadcast needed); rank 0's reply still decides
        loop/finish for everyone.  Every rank must own >= 1 map job
        (ranks without jobs could not shape their allreduce
        contribution)."""
        import torch

        from .gpu import dist as dx
        from .gpu.gradsum import allreduce_gradients

        t_start = gettime()
        rank, world = dx.world_info()
        gtask = Task(self.coord, key="task_gpu")
        while not self.finished:
            if rank == 0:
                gtask.create_collection(TASK_STATUS.WAIT, {
                    "fns": {"engine": "gradsum"},
                    "storage": "hbm", "result_ns": "result",
                }, self.iteration)
            jobs = self._collect_taskfn_jobs()
            mine = [kv for i, kv in enumerate(jobs) if i % world == rank]
            if not mine:
                raise RuntimeError(
                    f"gradsum engine: rank {rank} has no map jobs "
                    f"({len(jobs)} jobs, world {world}) — every rank "
                    "must contribute to the gradient allreduce")
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.MAP)
            acc = None
            for k, v in mine:
                g = self.fns.mapfn_gpu_grads(k, v)
                if acc is None:
                    acc = {n: t.detach().clone() for n, t in g.items()}
                else:
                    for n, t in g.items():
                        acc[n] += t
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.REDUCE)
            summed = allreduce_gradients(acc)
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.FINISHED)
            pairs = [(n, [summed[n]]) for n in sorted(summed)]
            # finalfn on EVERY rank with identical pairs (replica-sync
            # update); rank 0's decision wins
            reply = True
            if self.fns.finalfn is not None:
                reply = self.fns.finalfn(iter(pairs))
            if world > 1:
                import torch.distributed as td
                box = [reply]
                td.broadcast_object_list(box, src=0)
                reply = box[0]
            if reply == "loop":
                self.iteration += 1
            else:
                self.finished = True
        self.stats.update({
            "tier": "gpu", "engine": "gradsum",
            "map_failed": 0, "reduce_failed": 0,
            "iterations": self.iteration,
            "total_time": gettime() - t_start,
        })
        self.print_stats()

    def _loop_gpu_index(self) -> None:
        """Inverted-index GPU engine: mapfn_gpu stages each map job's
        raw bytes (one job = one document); the fused composite
        tokenizer + bucketized count + doc-then-hash sorts
        (gpu/inverted_index.py) build word -> [(doc, tf)] postings.

        Jobs are assigned to ranks in CONTIGUOUS blocks (not
        round-robin) so global doc ids are rank-contiguous
        (doc_base = this rank's first job index) and postings exchanged
        between ranks stay globally meaningful; finalfn receives
        (word, [(task_key, tf), ...]) with doc ids decoded back to the
        taskfn keys."""
        import numpy as np
        import torch

        from .gpu import dist as dx
        from .gpu.inverted_index import InvertedIndexJob

        t_start = gettime()
        rank, world = dx.world_info()
        device = (torch.device("cuda", torch.cuda.current_device())
                  if torch.cuda.is_available() else torch.device("cpu"))
        gtask = Task(self.coord, key="task_gpu")
        staged = None
        while not self.finished:
            if rank == 0:
                gtask.create_collection(TASK_STATUS.WAIT, {
                    "fns": {"engine": "inverted_index"},
                    "storage": "hbm", "result_ns": "result",
                }, self.iteration)
            jobs = self._collect_taskfn_jobs()
            per = (len(jobs) + world - 1) // world
            lo = min(rank * per, len(jobs))
            hi = min(lo + per, len(jobs))
            mine = jobs[lo:hi]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.MAP)
            sig = [k for k, _ in mine]
            if staged is None or staged[0] != sig:
                blobs = [self.fns.mapfn_gpu(k, v) for k, v in mine]
                splits = []
                off = 0
                for b in blobs:
                    splits.append((off, off + len(b)))
                    off += len(b) + 1
                joined = b"\n".join(bytes(b) for b in blobs)
                text = torch.from_numpy(
                    np.frombuffer(joined, dtype=np.uint8).copy()).to(device)
                staged = (sig, text, splits)
            _, text, splits = staged
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.REDUCE)
            idx = InvertedIndexJob(device, doc_base=lo).run(text, splits)
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.FINISHED)
            keys = [k for k, _ in jobs]  # global doc id -> taskfn key
            pairs = [
                (w.decode("utf-8", "surrogateescape"),
                 [(keys[d], tf) for d, tf in postings])
                for w, postings in idx.pair_iterator(order="lex")
            ]
            reply = self._gpu_finalize_round(pairs, rank, world,
                                             sort_key=lambda kv: kv[0])
            if reply == "loop":
                self.iteration += 1
                self._log(f"iterative loop -> iteration {self.iteration}")
            else:
                self.finished = True
        self.stats.update({
            "tier": "gpu", "engine": "inverted_index",
            "map_failed": 0, "reduce_failed": 0,
            "total_time": gettime() - t_start,
        })
        self.print_stats()

    def _loop_gpu_sort(self) -> None:
        """Distributed-sort GPU engine (TeraSort family): the task's
        emitted (key, payload) columns are staged per rank and sorted
        globally — one top-byte radix partition pass + xGMI all-to-all
        + local LSD radix sort (gpu/terasort.py).  Rank r owns the r-th
        contiguous range of the key space, so concatenating rank
        results in rank order IS global order; finalfn receives the
        pairs in that order (the reference's sorted-output guarantee,
        partition-major x in-partition order, server.lua:360-385).

        Payloads are one i64 column; gpu_key_decode (optional) maps
        result payloads back to user values at the finalfn boundary."""
        import torch

        from .gpu import dist as dx
        from .gpu.terasort import TeraSortJob

        t_start = gettime()
        rank, world = dx.world_info()
        device = (torch.device("cuda", torch.cuda.current_device())
                  if torch.cuda.is_available() else torch.device("cpu"))
        decode = self.fns.gpu_key_decode or (lambda p: p)
        gtask = Task(self.coord, key="task_gpu")
        staged = None
        while not self.finished:
            if rank == 0:
                gtask.create_collection(TASK_STATUS.WAIT, {
                    "fns": {"engine": "terasort"},
                    "storage": "hbm", "result_ns": "result",
                }, self.iteration)
            jobs = self._collect_taskfn_jobs()
            mine = [kv for i, kv in enumerate(jobs) if i % world == rank]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.MAP)
            sig = [k for k, _ in mine]
            if staged is None or staged[0] != sig:
                kcols, vcols = [], []
                for k, v in mine:
                    ks, vs = self.fns.mapfn_gpu_pairs(k, v)
                    kcols.append(torch.as_tensor(ks, dtype=torch.int64))
                    vcols.append(torch.as_tensor(vs, dtype=torch.int64))
                keys = (torch.cat(kcols).to(device) if kcols else
                        torch.empty(0, dtype=torch.int64, device=device))
                pays = (torch.cat(vcols).to(device) if vcols else
                        torch.empty(0, dtype=torch.int64, device=device))
                staged = (sig, keys, pays)
            _, keys, pays = staged
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.REDUCE)
            sk, sv = TeraSortJob(device).run(keys, pays)
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.FINISHED)
            pairs = [(k, [decode(p)]) for k, p in
                     zip(sk.cpu().tolist(), sv.cpu().tolist())]
            # rank-major concatenation IS global order: no re-sort
            reply = self._gpu_finalize_round(pairs, rank, world)
            if reply == "loop":
                self.iteration += 1
                self._log(f"iterative loop -> iteration {self.iteration}")
            else:
                self.finished = True
        self.stats.update({
            "tier": "gpu", "engine": "terasort",
            "map_failed": 0, "reduce_failed": 0,
            "total_time": gettime() - t_start,
        })
        self.print_stats()

    def _loop_gpu_join(self) -> None:
        """Equi-join GPU engine: each map job stages rows of ONE of two
        relations — mapfn_gpu_pairs(key, value) -> (keys, vals, side),
        side 0 = left, 1 = right — and the reduce pairs the rows of every
        key (gpu/join.py: stable sorts, mulhi-partitioned all-to-all of
        both sides, ops.join_sorted).  reducefn_gpu picks the join:
        "join" (inner), "join_left", "join_semi", "join_anti".

        finalfn receives, per key in global u64 key order,
        (gpu_key_decode(key), [(lval, rval), ...]) — rval None on the
        unmatched rows of join_left — or (key, [lval, ...]) under semi
        and anti.  Rank r owns the r-th contiguous range of the key space
        (mulhi is monotonic), so the rank-major concatenation is already
        that order.

        Contract: int64-representable keys; one value column per side,
        its dtype uniform across the side's map jobs (float -> f64, int
        -> i64)."""
        import torch

        from .gpu import dist as dx
        from .gpu.join import JoinJob

        t_start = gettime()
        rank, world = dx.world_info()
        device = (torch.device("cuda", torch.cuda.current_device())
                  if torch.cuda.is_available() else torch.device("cpu"))
        op = self.fns.reducefn_gpu
        how = self.GPU_JOIN_REDUCERS[op]
        pairwise = how in ("inner", "left")
        decode = self.fns.gpu_key_decode or (lambda k: k)
        gtask = Task(self.coord, key="task_gpu")
        staged = None  # (job signature, lk, lv, rk, rv) — iteration reuse
        while not self.finished:
            if rank == 0:
                gtask.create_collection(TASK_STATUS.WAIT, {
                    "fns": {"engine": f"join:{how}"},
                    "storage": "hbm", "result_ns": "result",
                }, self.iteration)
            jobs = self._collect_taskfn_jobs()
            mine = [kv for i, kv in enumerate(jobs) if i % world == rank]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.MAP)
            sig = [k for k, _ in mine]
            if staged is None or staged[0] != sig:
                kcols = ([], [])
                vcols = ([], [])
                for k, v in mine:
                    out = self.fns.mapfn_gpu_pairs(k, v)
                    if not (isinstance(out, (tuple, list))
                            and len(out) == 3 and out[2] in (0, 1)):
                        raise ValueError(
                            "mapfn_gpu_pairs must return (keys, vals, side) "
                            f"under reducefn_gpu={op!r}, side 0 for the "
                            "left relation and 1 for the right; job "
                            f"{k!r} returned "
                            + (f"a {len(out)}-tuple"
                               if isinstance(out, (tuple, list))
                               else type(out).__name__))
                    ks, vs, side = out
                    kcols[side].append(torch.as_tensor(ks,
                                                       dtype=torch.int64))
                    # floats stage as f64 from the start (as_tensor's
                    # default f32 would round them before the widening);
                    # an empty list is f32 to torch and decides nothing
                    vt = torch.as_tensor(vs)
                    vcols[side].append(
                        torch.as_tensor(vs, dtype=torch.float64)
                        if vt.is_floating_point() and vt.numel()
                        else vt.to(torch.int64))
                # a rank may stage nothing of a side yet receive its rows
                # in the shuffle: the ranks agree on each side's dtype
                isf = torch.tensor(
                    [int(any(c.is_floating_point() for c in vcols[s]))
                     for s in (0, 1)], dtype=torch.int64, device=device)
                if world > 1:
                    import torch.distributed as td
                    td.all_reduce(isf, op=td.ReduceOp.MAX)
                cols = []
                for s, f in zip((0, 1), isf.cpu().tolist()):
                    dt = torch.float64 if f else torch.int64
                    cols.append(torch.cat(kcols[s]).to(device) if kcols[s]
                                else torch.empty(0, dtype=torch.int64,
                                                 device=device))
                    cols.append(torch.cat(vcols[s]).to(dt).to(device)
                                if vcols[s]
                                else torch.empty(0, dtype=dt, device=device))
                staged = (sig, *cols)
            _, lk, lv, rk, rv = staged
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.REDUCE)
            res = JoinJob(device, how=how).run(lk, lv, rk, rv)
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.FINISHED)
            # one tolist() per column, then group the rows of each key
            keys = res.keys.cpu().tolist()
            rows = res.lvals.cpu().tolist()
            if pairwise:
                rvs = res.rvals.cpu().tolist()
                if how == "left":
                    rvs = [r if m else None for r, m in
                           zip(rvs, res.matched.cpu().tolist())]
                rows = list(zip(rows, rvs))
            pairs = []
            last = None
            for k, row in zip(keys, rows):
                if not pairs or k != last:
                    pairs.append((decode(k), []))
                    last = k
                pairs[-1][1].append(row)
            # rank-major concatenation IS global key order: no re-sort
            reply = self._gpu_finalize_round(pairs, rank, world)
            if reply == "loop":
                self.iteration += 1
                self._log(f"iterative loop -> iteration {self.iteration}")
            else:
                self.finished = True
        self.stats.update({
            "tier": "gpu", "engine": "join",
            "map_failed": 0, "reduce_failed": 0,
            "total_time": gettime() - t_start,
        })
        self.print_stats()

    def _loop_gpu_group(self) -> None:
        """Order-statistics GPU engine: the task's emitted (key, value)
        pairs are staged as device columns (mapfn_gpu_pairs, as for the
        keyed-reduce engine), grouped by key with the values of every key
        in order (gpu/grouped.py: sort, mulhi-partitioned all-to-all,
        ops.sort_values_in_groups) and reduced by reducefn_gpu:

          "group"                  (key, [values ascending])
          "median", one quantile   (key, [v])
          several quantiles        (key, [(v1, ..., vQ)])
          "topk:K" / "bottomk:K"   (key, [v1, ..., vm]), m = min(K, len),
                                   descending / ascending
          "distinct"               (key, [count])

        Quantiles pick the value at index (N * (len - 1)) // D of the
        ordered list.  topk, bottomk and distinct trim the lists before
        the exchange (GroupedValuesJob combine).  finalfn receives the
        pairs in global u64 key order: rank r owns the r-th contiguous
        range of the key space.

        Contract: int64-representable keys; the value dtype uniform across
        ranks (float -> f64, int -> i64)."""
        import torch

        from .gpu import dist as dx
        from .gpu.grouped import GroupedValuesJob

        t_start = gettime()
        rank, world = dx.world_info()
        device = (torch.device("cuda", torch.cuda.current_device())
                  if torch.cuda.is_available() else torch.device("cpu"))
        name = self.fns.reducefn_gpu
        op, arg = self.parse_group_reducer(name)
        combine = {"topk": ("topk", arg), "bottomk": ("bottomk", arg),
                   "distinct": "distinct"}.get(op)
        decode = self.fns.gpu_key_decode or (lambda k: k)
        gtask = Task(self.coord, key="task_gpu")
        staged = None  # (job signature, keys, vals) — iteration reuse
        while not self.finished:
            if rank == 0:
                gtask.create_collection(TASK_STATUS.WAIT, {
                    "fns": {"engine": f"group:{op}"},
                    "storage": "hbm", "result_ns": "result",
                }, self.iteration)
            jobs = self._collect_taskfn_jobs()
            mine = [kv for i, kv in enumerate(jobs) if i % world == rank]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.MAP)
            sig = [k for k, _ in mine]
            if staged is None or staged[0] != sig:
                kcols, vcols = [], []
                for k, v in mine:
                    ks, vs = self.fns.mapfn_gpu_pairs(k, v)
                    kcols.append(torch.as_tensor(ks, dtype=torch.int64))
                    # floats stage as f64 from the start: as_tensor's
                    # default (f32) would round them before the widening
                    vt = torch.as_tensor(vs)
                    vcols.append(torch.as_tensor(vs, dtype=torch.float64)
                                 if vt.is_floating_point()
                                 else vt.to(torch.int64))
                if kcols:
                    keys = torch.cat(kcols).to(device)
                    vals = torch.cat(vcols).to(device)
                else:
                    keys = torch.empty(0, dtype=torch.int64, device=device)
                    vals = torch.empty(0, dtype=torch.float64,
                                       device=device)
                staged = (sig, keys, vals)
            _, keys, vals = staged
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.REDUCE)
            res = GroupedValuesJob(device, combine=combine).run(keys, vals)
            ukeys = [decode(int(k)) for k in res.keys.cpu().tolist()]
            if op == "group":
                lists = [vs for _, vs in res.to_host()]
            elif op in ("median", "quantile"):
                rows = res.quantiles(arg or [(1, 2)]).cpu().tolist()
                lists = [[r[0]] if len(r) == 1 else [tuple(r)] for r in rows]
            elif op == "distinct":
                lists = [[c] for c in res.distinct().cpu().tolist()]
            else:
                top, m = res.topk(arg, largest=(op == "topk"))
                lists = [r[:c] for r, c in zip(top.cpu().tolist(),
                                               m.cpu().tolist())]
            pairs = list(zip(ukeys, lists))
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.FINISHED)
            # rank-major concatenation IS global key order: no re-sort
            reply = self._gpu_finalize_round(pairs, rank, world)
            if reply == "loop":
                self.iteration += 1
                self._log(f"iterative loop -> iteration {self.iteration}")
            else:
                self.finished = True
        self.stats.update({
            "tier": "gpu", "engine": f"group:{op}",
            "map_failed": 0, "reduce_failed": 0,
            "total_time": gettime() - t_start,
        })
        self.print_stats()

    def _loop_gpu_window(self) -> None:
        """Running-aggregate GPU engine: the task's emitted rows are staged
        as device columns (mapfn_gpu_pairs), grouped by key with the rows of
        every key in order (gpu/window.py: sort, mulhi-partitioned
        all-to-all, ops.sort_values_in_groups with the row permutation) and
        reduced by reducefn_gpu:

          "cumsum" / "cummin" / "cummax"
              mapfn_gpu_pairs returns (keys, order, vals); finalfn receives
              (key, [(order, running), ...]), the rows ascending by
              (order, value) and running = the sum / min / max of the
              values up to and including the row (ops.scan_by_key_sorted)
          "sessions:GAP"
              mapfn_gpu_pairs returns (keys, times); finalfn receives
              (key, [(start, end, count), ...]), one triple per session: a
              row opens a session when it starts its key or its time
              exceeds the previous one by more than GAP
          "rolling:OP:PRE[,fol=N][,rows]"
              OP = sum / min / max / mean: mapfn_gpu_pairs returns (keys,
              order, vals); OP = count: (keys, times).  finalfn receives
              (key, [(order, rolling), ...]), the rows ascending by
              (order, value) and rolling = OP over the row's frame
              (OrderedRows.rolling): the rows of the key whose order entry
              lies in [order - PRE, order + N], or with "rows" the PRE rows
              before it and the N rows behind it.  A range frame over a
              float order column raises the TypeError of ops.frame_bounds.

        finalfn receives the pairs in global u64 key order: rank r owns the
        r-th contiguous range of the key space.

        Contract: int64-representable keys; floats stage as f64 and ints as
        i64, uniformly across ranks; session times are integers."""
        import torch

        from .gpu import dist as dx
        from .gpu.window import WindowJob

        t_start = gettime()
        rank, world = dx.world_info()
        device = (torch.device("cuda", torch.cuda.current_device())
                  if torch.cuda.is_available() else torch.device("cpu"))
        name = self.fns.reducefn_gpu
        op, arg = self.parse_window_reducer(name)
        two = op == "sessions" or (op == "rolling" and arg["op"] == "count")
        ncols = 2 if two else 3
        what = "(keys, times)" if two else "(keys, order, vals)"
        decode = self.fns.gpu_key_decode or (lambda k: k)
        gtask = Task(self.coord, key="task_gpu")
        staged = None  # (job signature, columns) — iteration reuse

        def stage(col):
            # floats stage as f64 from the start: as_tensor's default
            # (f32) would round them before the widening; an empty list
            # is f32 to torch and decides nothing
            t = torch.as_tensor(col)
            if t.is_floating_point() and t.numel():
                return torch.as_tensor(col, dtype=torch.float64)
            return t.to(torch.int64)

        while not self.finished:
            if rank == 0:
                gtask.create_collection(TASK_STATUS.WAIT, {
                    "fns": {"engine": f"window:{op}"},
                    "storage": "hbm", "result_ns": "result",
                }, self.iteration)
            jobs = self._collect_taskfn_jobs()
            mine = [kv for i, kv in enumerate(jobs) if i % world == rank]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.MAP)
            sig = [k for k, _ in mine]
            if staged is None or staged[0] != sig:
                parts = [[] for _ in range(ncols)]
                for k, v in mine:
                    out = self.fns.mapfn_gpu_pairs(k, v)
                    if not (isinstance(out, (tuple, list))
                            and len(out) == ncols):
                        raise ValueError(
                            f"mapfn_gpu_pairs must return {what} under "
                            f"reducefn_gpu={name!r}; job {k!r} returned "
                            + (f"a {len(out)}-tuple"
                               if isinstance(out, (tuple, list))
                               else type(out).__name__))
                    parts[0].append(torch.as_tensor(out[0],
                                                    dtype=torch.int64))
                    for c in range(1, ncols):
                        parts[c].append(stage(out[c]))
                # a rank may stage nothing yet receive rows in the
                # shuffle: the ranks agree on each column's dtype
                isf = torch.tensor(
                    [int(any(t.is_floating_point() for t in parts[c]))
                     for c in range(ncols)], dtype=torch.int64,
                    device=device)
                if world > 1:
                    import torch.distributed as td
                    td.all_reduce(isf, op=td.ReduceOp.MAX)
                cols = []
                for c, f in enumerate(isf.cpu().tolist()):
                    dt = torch.float64 if f else torch.int64
                    cols.append(torch.cat(parts[c]).to(dt).to(device)
                                if parts[c]
                                else torch.empty(0, dtype=dt, device=device))
                staged = (sig, cols)
            cols = staged[1]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.REDUCE)
            res = WindowJob(device).run(*cols)
            if op == "sessions":
                host = res.sessions(arg).to_host()
            else:
                if op == "rolling":
                    run = res.rolling(arg["op"], arg["preceding"],
                                      arg["following"], arg["unit"])
                else:
                    run = res.scan(self.GPU_WINDOW_REDUCERS[op])
                run = run.cpu().tolist()
                off = res.offsets.cpu().tolist()
                rows = list(zip(res.order.cpu().tolist(), run))
                host = [(k, rows[off[s]:off[s + 1]])
                        for s, k in enumerate(res.keys.cpu().tolist())]
            pairs = [(decode(int(k)), rows) for k, rows in host]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.FINISHED)
            # rank-major concatenation IS global key order: no re-sort
            reply = self._gpu_finalize_round(pairs, rank, world)
            if reply == "loop":
                self.iteration += 1
                self._log(f"iterative loop -> iteration {self.iteration}")
            else:
                self.finished = True
        self.stats.update({
            "tier": "gpu", "engine": f"window:{op}",
            "map_failed": 0, "reduce_failed": 0,
            "total_time": gettime() - t_start,
        })
        self.print_stats()

    def _loop_gpu_asof(self) -> None:
        """As-of join GPU engine: each map job stages rows of ONE of two
        time-ordered relations — mapfn_gpu_pairs(key, value) -> (keys,
        times, vals, side), side 0 = left, 1 = right — and the reduce pairs
        every left row with one right row of its key (gpu/asof.py: both
        sides arranged by (key, time, value) and mulhi-shuffled by
        WindowJob, ops.asof_sorted).  reducefn_gpu is "join_asof",
        optionally followed by ":" and options (parse_asof_reducer):
        backward / forward / nearest, strict, inner, tol=N.

        finalfn receives, per key in global u64 key order,
        (gpu_key_decode(key), [(ltime, lval, rtime, rval), ...]), the rows
        ascending by (ltime, lval); rtime and rval are None on unmatched
        rows, which "inner" drops.  Rank r owns the r-th contiguous range
        of the key space (mulhi is monotonic), so the rank-major
        concatenation is already that order.

        Contract: int64-representable keys; one time and one value column
        per side, floats staged as f64 and ints as i64, uniformly across
        ranks; the two sides' times share one dtype."""
        import torch

        from .gpu import dist as dx
        from .gpu.asof import AsofJoinJob

        t_start = gettime()
        rank, world = dx.world_info()
        device = (torch.device("cuda", torch.cuda.current_device())
                  if torch.cuda.is_available() else torch.device("cpu"))
        name = self.fns.reducefn_gpu
        opts = self.parse_asof_reducer(name)
        decode = self.fns.gpu_key_decode or (lambda k: k)
        gtask = Task(self.coord, key="task_gpu")
        staged = None  # (job signature, six columns) — iteration reuse

        def stage(col):
            # floats stage as f64 from the start: as_tensor's default
            # (f32) would round them before the widening; an empty list
            # is f32 to torch and decides nothing
            t = torch.as_tensor(col)
            if t.is_floating_point() and t.numel():
                return torch.as_tensor(col, dtype=torch.float64)
            return t.to(torch.int64)

        while not self.finished:
            if rank == 0:
                gtask.create_collection(TASK_STATUS.WAIT, {
                    "fns": {"engine": f"asof:{opts['direction']}"},
                    "storage": "hbm", "result_ns": "result",
                }, self.iteration)
            jobs = self._collect_taskfn_jobs()
            mine = [kv for i, kv in enumerate(jobs) if i % world == rank]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.MAP)
            sig = [k for k, _ in mine]
            if staged is None or staged[0] != sig:
                # parts[side][column]: keys, times, vals
                parts = ([[], [], []], [[], [], []])
                for k, v in mine:
                    out = self.fns.mapfn_gpu_pairs(k, v)
                    if not (isinstance(out, (tuple, list))
                            and len(out) == 4 and out[3] in (0, 1)):
                        raise ValueError(
                            "mapfn_gpu_pairs must return (keys, times, vals, "
                            f"side) under reducefn_gpu={name!r}, side 0 for "
                            "the left relation and 1 for the right; job "
                            f"{k!r} returned "
                            + (f"a {len(out)}-tuple"
                               if isinstance(out, (tuple, list))
                               else type(out).__name__))
                    side = out[3]
                    parts[side][0].append(torch.as_tensor(out[0],
                                                          dtype=torch.int64))
                    parts[side][1].append(stage(out[1]))
                    parts[side][2].append(stage(out[2]))
                # a rank may stage nothing of a side yet receive its rows
                # in the shuffle: the ranks agree on each column's dtype
                isf = torch.tensor(
                    [int(any(t.is_floating_point() for t in parts[s][c]))
                     for s in (0, 1) for c in (1, 2)], dtype=torch.int64,
                    device=device)
                if world > 1:
                    import torch.distributed as td
                    td.all_reduce(isf, op=td.ReduceOp.MAX)
                isf = isf.cpu().tolist()
                if isf[0] != isf[2]:
                    # the same vector on every rank: all of them raise
                    raise TypeError(
                        "the two relations' times must share one dtype under "
                        f"reducefn_gpu={name!r}: the left times are "
                        f"{'float' if isf[0] else 'int'}, the right ones "
                        f"{'float' if isf[2] else 'int'}")
                cols = []
                for s in (0, 1):
                    for c in range(3):
                        f = isf[2 * s + c - 1] if c else 0
                        dt = torch.float64 if f else torch.int64
                        cols.append(
                            torch.cat(parts[s][c]).to(dt).to(device)
                            if parts[s][c]
                            else torch.empty(0, dtype=dt, device=device))
                staged = (sig, cols)
            cols = staged[1]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.REDUCE)
            res = AsofJoinJob(device, **opts).run(*cols)
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.FINISHED)
            # one tolist() per column, then group the rows of each key
            keys = res.keys.cpu().tolist()
            rts = res.rtimes.cpu().tolist()
            rvs = res.rvals.cpu().tolist()
            if res.matched is not None:
                ma = res.matched.cpu().tolist()
                rts = [t if m else None for t, m in zip(rts, ma)]
                rvs = [v if m else None for v, m in zip(rvs, ma)]
            rows = zip(res.ltimes.cpu().tolist(), res.lvals.cpu().tolist(),
                       rts, rvs)
            pairs = []
            last = None
            for k, row in zip(keys, rows):
                if not pairs or k != last:
                    pairs.append((decode(k), []))
                    last = k
                pairs[-1][1].append(row)
            # rank-major concatenation IS global key order: no re-sort
            reply = self._gpu_finalize_round(pairs, rank, world)
            if reply == "loop":
                self.iteration += 1
                self._log(f"iterative loop -> iteration {self.iteration}")
            else:
                self.finished = True
        self.stats.update({
            "tier": "gpu", "engine": "asof",
            "map_failed": 0, "reduce_failed": 0,
            "total_time": gettime() - t_start,
        })
        self.print_stats()

    # ------------------------------------------------------------ map phase
    def _loop_gpu_graph(self) -> None:
        """Resident-graph GPU engine: each map job stages edges as two key
        columns — mapfn_gpu_pairs(key, value) -> (src, dst) — and the whole
        iteration runs on the device (gpu/graph.py): the graph is built once
        as a CSR by destination and every iteration is one
        ops.graph_propagate pass, so the Python boundary is crossed once
        per round, not once per iteration.

          "pagerank[:d=D][,iters=N][,tol=T]"
              finalfn receives (node, [rank]) for every node of either
              column, after at most N iterations or the first one whose
              |r' - r|_1 <= T
          "components"
              the edges are taken as undirected; finalfn receives
              (node, [label]), the label being the smallest key of the
              node's component in u64 order

        finalfn receives the pairs in global u64 key order: rank r emits
        the r-th contiguous slice of the nodes.  When finalfn returns
        "loop" and the job signature is unchanged the engine keeps the
        Graph and continues the ranks for up to N more iterations; a
        changed signature rebuilds.

        Contract: int64-representable keys."""
        import torch

        from .gpu import dist as dx
        from .gpu.graph import GraphJob

        t_start = gettime()
        rank, world = dx.world_info()
        device = (torch.device("cuda", torch.cuda.current_device())
                  if torch.cuda.is_available() else torch.device("cpu"))
        name = self.fns.reducefn_gpu
        opts = self.parse_graph_reducer(name)
        algo = opts["algo"]
        decode = self.fns.gpu_key_decode or (lambda k: k)
        gtask = Task(self.coord, key="task_gpu")
        staged = None  # (job signature, Graph, PageRankResult) — reuse
        iterations = 0

        while not self.finished:
            if rank == 0:
                gtask.create_collection(TASK_STATUS.WAIT, {
                    "fns": {"engine": f"graph:{algo}"},
                    "storage": "hbm", "result_ns": "result",
                }, self.iteration)
            jobs = self._collect_taskfn_jobs()
            mine = [kv for i, kv in enumerate(jobs) if i % world == rank]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.MAP)
            sig = [k for k, _ in mine]
            if staged is None or staged[0] != sig:
                parts = [[], []]
                for k, v in mine:
                    out = self.fns.mapfn_gpu_pairs(k, v)
                    if not (isinstance(out, (tuple, list))
                            and len(out) == 2):
                        raise ValueError(
                            "mapfn_gpu_pairs must return (src, dst) under "
                            f"reducefn_gpu={name!r}; job {k!r} returned "
                            + (f"a {len(out)}-tuple"
                               if isinstance(out, (tuple, list))
                               else type(out).__name__))
                    for c in range(2):
                        parts[c].append(torch.as_tensor(out[c],
                                                        dtype=torch.int64))
                cols = [torch.cat(p).to(device) if p
                        else torch.empty(0, dtype=torch.int64, device=device)
                        for p in parts]
                graph = GraphJob(device).run(
                    cols[0], cols[1], symmetric=algo == "components")
                staged = (sig, graph, None)
            _, graph, pr = staged
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.REDUCE)
            if algo == "components":
                vals, rounds = graph.components()
                iterations += rounds
            else:
                before = pr.iterations if pr is not None else 0
                pr = (graph.pagerank(opts["damping"], opts["iters"],
                                     opts["tol"]) if pr is None
                      else pr.more(opts["iters"]))
                staged = (sig, graph, pr)
                vals = pr.ranks
                iterations += pr.iterations - before
            a, b = graph.owned()
            pairs = [(decode(int(k)), [v]) for k, v in zip(
                graph.nodes[a:b].cpu().tolist(), vals[a:b].cpu().tolist())]
            if rank == 0:
                gtask.set_task_status(TASK_STATUS.FINISHED)
            # rank-major concatenation IS global key order: no re-sort
            reply = self._gpu_finalize_round(pairs, rank, world)
            if reply == "loop":
                self.iteration += 1
                self._log(f"iterative loop -> iteration {self.iteration}")
            else:
                self.finished = True
        self.stats.update({
            "tier": "gpu", "engine": f"graph:{algo}",
            "graph_iterations": iterations,
            "map_failed": 0, "reduce_failed": 0,
            "total_time": gettime() - t_start,
        })
        self.print_stats()

    def _prepare_map(self) -> None:
        """server_prepare_map (server.lua:249-276): run taskfn(emit), check
        key uniqueness and value size, insert map job docs, set phase MAP."""
        done = self.task.written_ids(Task.MAP_JOBS)
        self.task.remove_pending(Task.MAP_JOBS)
        jobs: List[dict] = []
        seen = set(done)
        order: List[str] = list(self.task.coord.get_ids(Task.MAP_JOBS))

        def emit(key, value):
            k = str(key)
            if k in seen:
                if k in done:
                    return  # restored: already WRITTEN, never redo
                raise ValueError(f"duplicate taskfn key {key!r} "
                                 "(server.lua:258-261)")
            seen.add(k)
            assert_check(value)
            import pickle
            if len(pickle.dumps(value)) > MAX_TASKFN_VALUE_SIZE:
                raise ValueError(
                    f"taskfn value for key {key!r} exceeds "
                    f"{MAX_TASKFN_VALUE_SIZE} bytes (server.lua:262-267)")
            jobs.append(make_job(k, value))
            order.append(k)

        self.fns.taskfn(emit)
        for j in jobs:
            self.task.coord.set_doc(f"{Task.MAP_JOBS}/{j['_id']}", j)
        self.task.coord.set_ids(Task.MAP_JOBS, order)
        self.task.set_task_status(TASK_STATUS.MAP)
        self._log(f"map phase: {len(jobs)} jobs "
                  f"({len(done)} restored as WRITTEN)")

    # --------------------------------------------------------- reduce phase
    def _prepare_reduce(self) -> None:
        """server_prepare_reduce (server.lua:279-329): scan the shuffle
        namespace for map_results.P<p>.M<m> spills, build one reduce job
        per partition, set phase REDUCE."""
        done = self.task.written_ids(Task.RED_JOBS)
        self.task.remove_pending(Task.RED_JOBS)
        names = self.fs.list(r"^map_results\.P\d+\.M.*$")
        parts: Dict[int, int] = {}
        rx = re.compile(r"^map_results\.P(\d+)\.M(.+)$")
        for n in names:
            m = rx.match(n)
            if m:
                p = int(m.group(1))
                parts[p] = parts.get(p, 0) + 1
        jobs = []
        order = list(self.task.coord.get_ids(Task.RED_JOBS))
        for p in sorted(parts):
            jid = str(p)
            if jid in done:
                continue
            jobs.append(make_job(jid, {
                "part": p,
                "file": f"map_results.P{p}",
                "result": f"{self.params['result_ns']}.P{p}",
                "mappers": parts[p],
            }))
            order.append(jid)
        for j in jobs:
            self.task.coord.set_doc(f"{Task.RED_JOBS}/{j['_id']}", j)
        self.task.coord.set_ids(Task.RED_JOBS, order)
        self.task.set_task_status(TASK_STATUS.REDUCE)
        nfiles = sum(parts.values())
        self._log(f"reduce phase: {len(jobs)} partitions over "
                  f"{nfiles} shuffle files")

    # ---------------------------------------------------------- poll engine
    def _poll_until_done(self, ns: str, phase: str) -> None:
        """Progress poller (make_task_coroutine_wrap, server.lua:186-234):
        promote exhausted BROKEN jobs to FAILED, requeue stale RUNNING jobs
        (heartbeat), print % progress, drain the error channel."""
        last_pct = -1
        last_progress = (-1, gettime())
        while True:
            self.task.promote_broken(ns)
            if self.heartbeat_timeout:
                n = self.task.requeue_stale(ns, self.heartbeat_timeout)
                if n:
                    self._log(f"requeued {n} stale {phase} jobs")
            errors, self._errors_drained = self.coord.get_errors(
                self._errors_drained)
            for e in errors:
                self._log(f"worker error [{e['who']}]: {e['msg']}")
            written, failed, total = self.task.count_done(ns)
            if written + failed != last_progress[0]:
                last_progress = (written + failed, gettime())
            elif (self.stall_timeout
                  and gettime() - last_progress[1] > self.stall_timeout):
                # no progress for stall_timeout: the worker pool is likely
                # depleted (each worker quits after MAX_WORKER_RETRIES
                # distinct failures) — force-fail the stuck BROKEN jobs so
                # the task completes with a failure count instead of
                # polling forever (liveness fix over the reference)
                n = self.task.force_fail_incomplete(ns)
                if n:
                    self._log(f"stall: force-failed {n} {phase} jobs")
                last_progress = (written + failed, gettime())
            if total:
                pct = int(100 * (written + failed) / total)
                if pct != last_pct:
                    self._log(f"{phase} {pct:3d}% ({written} written, "
                              f"{failed} failed, {total} total)")
                    last_pct = pct
            if written + failed >= total:
                self.stats[f"{phase}_failed"] = failed
                return
            time.sleep(self.poll_interval)

    # --------------------------------------------------------------- stats
    def _compute_stats(self, ns: str, phase: str) -> None:
        """Aggregate per-job timing (server.lua compute_sum :177-183,
        compute_real_time :155-175: cluster time = max(written_time) -
        min(started_time))."""
        docs = [d for d in self.task.scan_jobs(ns)
                if d["status"] == STATUS.WRITTEN]
        if not docs:
            return
        cpu = sum(d["cpu_time"] for d in docs)
        real = sum(d["real_time"] for d in docs)
        started = min(d["started_time"] for d in docs if d["started_time"])
        written = max(d["written_time"] for d in docs if d["written_time"])
        self.stats[phase] = {
            "sum_cpu_time": cpu,
            "sum_real_time": real,
            "cluster_time": written - started,
            "jobs": len(docs),
        }

    def print_stats(self) -> None:
        """Stats block in the reference's report format (server.lua:557-602)."""
        for phase in ("map", "reduce"):
            s = self.stats.get(phase)
            if not s:
                continue
            self._log(f"{phase}: sum(cpu_time) {s['sum_cpu_time']:.2f} s  "
                      f"sum(real_time) {s['sum_real_time']:.2f} s  "
                      f"cluster_time {s['cluster_time']:.2f} s  "
                      f"jobs {s['jobs']}  failed "
                      f"{self.stats.get(phase + '_failed', 0)}")
        if "total_time" in self.stats:
            self._log(f"total server time {self.stats['total_time']:.2f} s")

    # --------------------------------------------------------------- final
    def _final(self) -> Any:
        """server_final (server.lua:348-413): stream all result.P<p> files
        sorted by partition into finalfn as a (key, values) iterator."""
        rns = self.params["result_ns"]
        names = self.fs.list(rf"^{re.escape(rns)}\.P\d+$")
        names.sort(key=lambda n: int(n.rsplit("P", 1)[1]))

        def pair_iterator():
            for n in names:
                yield from self.fs.records(n)

        reply = True
        if self.fns.finalfn is not None:
            reply = self.fns.finalfn(pair_iterator())
        if reply is True or reply == "loop":
            for n in names:
                self.fs.remove(n)
        return reply

    # ---------------------------------------------------------------- loop
    def loop(self) -> None:
        """Main driver loop (server.lua:466-611).  Tasks whose modules
        declare the GPU hooks (mapfn_gpu + builtin reducefn_gpu +
        assoc/comm flags) run entirely on the HIP engine; everything
        else takes the general host tier below."""
        assert self.params is not None, "configure() first"
        kind = self._gpu_engine_kind()
        if kind is not None:
            fn = {"bytes": self._loop_gpu,
                  "pairs": self._loop_gpu_pairs,
                  "sort": self._loop_gpu_sort,
                  "join": self._loop_gpu_join,
                  "group": self._loop_gpu_group,
                  "window": self._loop_gpu_window,
                  "asof": self._loop_gpu_asof,
                  "graph": self._loop_gpu_graph,
                  "index": self._loop_gpu_index,
                  "gradsum": self._loop_gpu_grads}[kind]
            try:
                return fn()
            except Exception as e:
                # durable failure record (the GPU-tier analogue of the
                # task doc a crashed reference server leaves behind,
                # server.lua:470-504): a restarted driver can see what
                # died and that a replay is needed
                try:
                    self.coord.set_doc("task_gpu_failure", {
                        "_id": "failure", "engine": kind,
                        "error": repr(e), "time": gettime()})
                except Exception:
                    pass
                raise
        t_start = gettime()
        # restore check (server.lua:470-504)
        self.task.update()
        skip_map = False
        if self.task.exists():
            st = self.task.status()
            if st == TASK_STATUS.FINISHED:
                self.task.drop_all()
            else:
                self._log("WARNING: TRYING TO RESTORE A BROKEN TASK "
                          "(server.lua:479)")
                self.iteration = self.task.iteration() or 1
                if st == TASK_STATUS.REDUCE:
                    skip_map = True

        while not self.finished:
            if not self.task.exists() or not skip_map:
                self.task.create_collection(TASK_STATUS.WAIT, self.params,
                                            self.iteration)
            if not skip_map:
                self._prepare_map()
                self._poll_until_done(Task.MAP_JOBS, "map")
                self._compute_stats(Task.MAP_JOBS, "map")
            skip_map = False
            self._prepare_reduce()
            self._poll_until_done(Task.RED_JOBS, "reduce")
            self._compute_stats(Task.RED_JOBS, "reduce")
            reply = self._final()
            if reply == "loop":
                self.iteration += 1
                self.task.drop_jobs()
                self._log(f"iterative loop -> iteration {self.iteration}")
            else:
                self.finished = True
        self.stats["total_time"] = gettime() - t_start
        # persist the stats sub-document in the task singleton
        # (server.lua:584-601 task:insert{stats})
        self.task.set_task_status(TASK_STATUS.FINISHED, stats=self.stats)
        self.task.drop_jobs()
        self.print_stats()

    def drop_all(self) -> None:
        self.task.update()
        self.task.drop_all()


def new(cnn_string: str = "local", db: str = "mr", **kw) -> Server:
    """server.new (server.lua:616-624)."""
    return Server(cnn_string, db, **kw)
