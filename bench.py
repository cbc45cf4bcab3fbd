#!/usr/bin/env python3
"""bench.py -- BASELINE.json metric on MI355X: trace-LDE + Merkle-commit of a 2^20 x 8 f64 trace at blowup 8.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--mode proofs|packed] [--ranks processes|threads]
                    [--dump-outputs DIR] [--full [--config cfg2|cfg3|cfg5|dowork] [--per-launch]]

A "step" is one pass of the hot path (Prover::build_trace_commitment, /root/reference/prover/src/lib.rs:615-670)
over one synthetic trace that is already resident in HBM: interpolate 8 columns -> evaluate over the 8 cosets into
the row-major LDE matrix -> hash 2^23 rows -> build the Merkle tree.

N > 1: one process per GPU.  As a plain command (`python bench.py --gpus 8`) this process only starts the ranks --
`python -m torch.distributed.run --nproc-per-node N bench.py ...` as child processes, before anything here touches
the GPU -- and passes their output and exit code through; started by torch.distributed.run itself (RANK in the
environment) it is a rank.
  --mode proofs (default; BASELINE.json configs[3]): every rank commits its own independent proof (weak scaling)
      and the step sequence ends with the path's one collective, an all-gather of the 32-byte roots over RCCL
      (wf_comm_all_gather_roots: the collective lives inside libwf_lde.so, behind the C ABI).
  --mode packed: ONE STARKPack commitment of 8 packed 2^20 x 8 traces, sharded by coset over the ranks
      (wf_trace_commit_sharded_dev; strong scaling).
--ranks threads (N > 1 as a plain command): ONE process, one host thread + one wf_ctx + one wf_comm per GPU on real
RCCL (ncclCommInitRank from N threads with one unique id) -- same steps, same gates, same JSON line; for boxes that
limit the processes per card.  The parent decides the route before anything touches the GPU and never re-executes.
WF_BENCH_BACKEND=gloo (processes) / loopback (threads) rehearses the multi-rank control flow on a box with fewer GPUs
than ranks: the ranks share the device and the bytes of the collectives travel over a torch.distributed gloo group /
through host memory (wf_transport).

A plain run sets up, warms up, times the K steps, writes the outputs of the last step if --dump-outputs is given and
prints the line; everything else the record holds is measured only under --full.

--full (off by default) adds the measurements that take runs of their own: the `alu` yardstick, `with_transfers`,
`cpu_baseline` (with its root-parity gate against the CPU oracle); and it admits the record's other workloads and
finer passes:
  --config (single GPU) prints the same line for the other workloads of the record: cfg3 (2^22 x 64 f64), cfg5 (f128
      2^18 x 10), dowork (the reference's example at its defaults: 512 packed f128 traces of 2^10); the headline stays cfg2.
  --per-launch: a separate pass after the timed region with an event per kernel launch.

--dump-outputs DIR: after the timed steps, rank 0 writes what its last step computed -- the arrays the caller of
wf_trace_commit_dev receives -- as DIR/<name>.npy: root (32 bytes), and a fixed, seeded sample of rows of nodes and
leaves (bytes as float32), of lde and polys (each u64 word as two exact 32-bit limbs, low first, in float64); at most
12 MiB per array.  The inputs are seeded, so two builds run with the same arguments can be compared output for output.

Rank 0 prints ONE JSON line (metric, value, unit, higher_is_better, dtype, ms_per_step, ...) with these extra objects:
  roofline       : dominant logical kernel, its algorithmic bytes per launch
                   / its HIP-event duration measured inside the timed region, against the 8 TB/s HBM peak
  alu            : (--full) the step against the time its butterflies and BLAKE3 compressions take at the rates the same
                   instruction sequences reach in isolation -- measured IN THIS RUN (csrc/yardstick.hip), with the clocks
                   both ran at
  cpu_baseline   : (--full) the CPU oracle (oracle/, "port" of the reference's concurrent path) timed on the host cores
                   on full commitments of the same workload (rank 0, N == 1 only)
  with_transfers : (--full) the same commitment through the host-buffer and the resident entry points (PCIe included;
                   N == 1 only, outside the timed region; never `value`)
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

LOG_R, LOG_B, N_COLS = 20, 3, 8   # the metric's configuration (cfg 2); --config selects another single-GPU workload
PACKED_TRACES = 8
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)

# Workloads.  cfg2 is the configuration BASELINE.json's metric is quoted on and the only one the driver's contract runs
# (python bench.py [--gpus N]); the others print the same JSON line for the record (profiles/r03_cfg3_*, r03_cfg5_*).
CONFIGS = {
    "cfg2": dict(field="f64", log_r=20, log_b=3, n_cols=8, n_traces=1,
                 label="BASELINE.json configs[1]: 2^20 rows x 8 cols f64, blowup 8, BLAKE3-256 Merkle"),
    "cfg3": dict(field="f64", log_r=22, log_b=3, n_cols=64, n_traces=1,
                 label="BASELINE.json configs[2], trace side: 2^22 rows x 64 cols f64, blowup 8 (16 GiB LDE)"),
    "cfg5": dict(field="f128", log_r=18, log_b=3, n_cols=10, n_traces=1,
                 label="BASELINE.json configs[4] substitute (SURVEY.md §8d): do_work-shaped f128 trace, 2^18 rows x 10 cols, blowup 8, path only"),
    "dowork": dict(field="f128", log_r=10, log_b=3, n_cols=10, n_traces=512,
                   label="the reference's own example at its defaults (examples/src/lib.rs:97-135): 512 packed do_work traces of "
                         "2^10 rows x 10 cols f128 under ONE tree (80-chunk rows), blowup 8"),
}


def row_compressions(row_bytes):
    """BLAKE3 compressions of one hashed row: 64-byte blocks, plus the parent nodes of a row longer than a chunk."""
    if row_bytes <= 1024:
        return max(1, (row_bytes + 63) // 64)
    chunks = (row_bytes + 1023) // 1024
    last = row_bytes - (chunks - 1) * 1024
    return (chunks - 1) * 16 + (last + 63) // 64 + (chunks - 1)


def work_model(log_r=LOG_R, log_b=LOG_B, c=N_COLS, e=8, n_traces=1):
    """algorithmic bytes and field operations of one commitment (n_traces packed traces)."""
    R, N = 1 << log_r, 1 << (log_r + log_b)
    beta = 1 << log_b
    C = c * n_traces
    bytes_k = {
        "interpolate": R * C * e + R * C * e,          # K1: read trace, write polys
        "evaluate": R * C * e + N * C * e,             # K2: read polys, write LDE
        "hash_rows": N * C * e + N * 32,               # K3: read LDE rows, write leaves
        "merkle": N * 32 + N * 32,                     # K4: read leaves, write nodes
    }
    b_alg = R * C * e * 2 + N * C * e + N * 32 * 2     # §8(d): each datum of the path exactly once
    butterflies = C * (R // 2) * log_r * (1 + beta)
    muls = butterflies + C * R + beta * C * R
    field_ops = 3 * butterflies + C * R + beta * C * R
    compressions = N * row_compressions(C * e) + (N - 1)
    return dict(bytes_per_kernel=bytes_k, b_alg=b_alg, field_ops=field_ops, modmuls=muls, compressions=compressions,
                butterflies=butterflies)


def gpu_clock_files(torch, dev_index):
    """hwmon files with the current shader clock of device dev_index (Hz), matched by PCI address; [] if unreadable."""
    import glob
    files = glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/freq1_input")
    try:
        pr = torch.cuda.get_device_properties(dev_index)
        addr = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}"
        mine = [f for f in files if addr in os.path.realpath(f)]
        if mine:
            return mine[:1]
    except Exception:  # noqa: BLE001 -- older torch: no PCI ids
        pass
    return files


class ClockSampler:
    """Reads the driver's current shader clock (hwmon freq1_input, what the SMU reports) in a thread while a measurement
    runs.  With several candidate cards (no PCI match) the highest reading of a sweep is the busy GPU: ours."""

    def __init__(self, files):
        import threading
        self.files, self.samples, self._stop = files, [], threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while not self._stop.is_set():
            best = 0
            for f in self.files:
                try:
                    best = max(best, int(open(f).read()))
                except (OSError, ValueError):
                    pass
            if best:
                self.samples.append(best / 1e6)

    def __enter__(self):
        if self.files:
            self._t.start()
        return self

    def __exit__(self, *a):
        self._stop.set()
        if self.files:
            self._t.join(timeout=2)

    def summary(self):
        if not self.samples:
            return None
        v = sorted(self.samples)
        return {"mean_mhz": round(sum(v) / len(v), 1), "min_mhz": v[0], "max_mhz": v[-1], "samples": len(v)}


def yardstick(torch, dev_index, clock_files, is64):
    """The integer-VALU rates of the path's own instruction sequences in isolation, measured NOW on this GPU
    (csrc/yardstick.hip: Goldilocks or f128 butterflies, BLAKE3 compressions; register-only loops, 8 waves per SIMD),
    each with the driver's shader-clock reading sampled while exactly that loop ran."""
    import ctypes as C
    from starkpack_winterfell_amd.build import yardstick_path
    path = yardstick_path()
    if not os.path.exists(path):
        return {"error": "libwf_yardstick.so has not been built"}
    Y = C.CDLL(path)
    Y.wf_yardstick_run.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double)]
    res = {}
    for name, which in (("butterflies", 0 if is64 else 1), ("blake3_compressions", 2)):
        out = (C.c_double * 2)()
        with ClockSampler(clock_files) as cs:
            rc = Y.wf_yardstick_run(dev_index, which, out)
        if rc:
            return {"error": f"wf_yardstick_run({which}) failed with {rc}"}
        res[name] = {"per_s": out[0], "kernel_ms": round(out[1], 3), "clock_driver": cs.summary()}
    return res


def rand_f64_dev(torch, n, seed, device):
    """n uniform Montgomery residues in [0, p) on the device (int64 storage of the u64 bit patterns)."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    v = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=device, generator=gen)
    bad = (v >> 32) == -1  # top 32 bits all ones: may be >= p = 2^64 - 2^32 + 1
    return torch.where(bad, v & 0x7FFFFFFFFFFFFFFF, v)


def rand_f128_dev(torch, n, seed, device):
    """n canonical elements of the 128-bit field (< 2^127 < p) as int64 pairs (lo, hi)."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    v = torch.randint(-2**63, 2**63 - 1, (n, 2), dtype=torch.int64, device=device, generator=gen)
    v[:, 1] &= 0x7FFFFFFFFFFFFFFF
    return v.reshape(-1)


def csrc_sha():
    """Digest of the kernel sources: profiles/traffic.json is only quoted for the kernels it was measured on."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "starkpack-winterfell_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".hpp")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def probe(cmd):
    """First line a toolchain probe prints, or None (cargo / rustc on the GPU box: BASELINE.md §3)."""
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=20)
        return (out.stdout or out.stderr).strip().splitlines()[0] if out.returncode == 0 else None
    except (OSError, subprocess.SubprocessError, IndexError):
        return None


def cpu_budget():
    """What this process may actually use of the host: the CPUs of its affinity mask AND the cgroup's CPU-time quota (a
    container handed "16 CPUs' worth" of a 128-thread host sees all 128 in its mask; 64 threads on such a quota are throttled
    by the scheduler, which is what a 15 % parallel efficiency looks like).  Returns (usable_threads, details)."""
    det = {"os_cpu_count": os.cpu_count()}
    try:
        det["affinity"] = len(os.sched_getaffinity(0))
    except AttributeError:
        det["affinity"] = os.cpu_count()
    quota = None
    try:  # cgroup v2
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        det["cgroup_cpu_max"] = f"{q} {per}"
        if q != "max":
            quota = int(q) / int(per)
    except (OSError, ValueError):
        try:  # cgroup v1
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            det["cgroup_cfs_quota_us"], det["cgroup_cfs_period_us"] = q, per
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            det["cgroup"] = "no cpu controller file readable"
    det["quota_cpus"] = quota
    usable = det["affinity"] or 1
    if quota:
        usable = max(1, min(usable, int(quota + 0.5)))
    return usable, det


def cpu_baseline(model, wl, traces_host, gpu_root=None, runs=5, warmups=2):
    """Full commitments of the bench workload (the very traces rank 0 committed on the GPU) with the threaded CPU
    oracle -- test infrastructure, used here only as the reported CPU baseline and as a last parity gate.  The C
    entry point is timed on preallocated outputs that the worker threads themselves faulted in (first touch in the warm-up
    run, same static partitioning in every run; no Python allocation inside the clock).
    Thread count: swept once over 8 / 16 / 32 / 64 (up to the affinity mask; the cgroup quota is reported next to it), the
    count with the best median is the one quoted.  traces_host: [n_traces][n_cols] arrays.  Phases (ms) are those of the
    median run; efficiency = the phase's compressions at THIS box's measured single-thread rate / threads / the phase."""
    usable, budget = cpu_budget()
    # libgomp reads these when liboracle.so (first user of the system libgomp in this process) is loaded
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")
    import numpy as np
    from oracle import oracle as O
    O.build()
    field = O.F64 if wl["field"] == "f64" else O.F128
    offset = 7 if wl["field"] == "f64" else 3
    data = [[np.ascontiguousarray(c) for c in t] for t in traces_host]
    N = 1 << (wl["log_r"] + wl["log_b"])
    leaf_comp = model["compressions"] - (N - 1)

    # this box's single-thread cost of one 2-to-1 hash (the figure the reference publishes, crypto/README.md:69-75)
    rng = np.random.default_rng(11)
    probe_leaves = rng.integers(0, 256, size=(1 << 16, 32), dtype=np.uint8)
    O.build_merkle_nodes(probe_leaves, 1)
    t0 = time.perf_counter()
    O.build_merkle_nodes(probe_leaves, 1)
    ns_single = (time.perf_counter() - t0) * 1e9 / ((1 << 16) - 1)

    def commit(threads, res):
        t0 = time.perf_counter()
        res = O.build_trace_commitment(field, data, 1, wl["log_r"], wl["log_b"], offset, threads=threads, out=res)
        return (time.perf_counter() - t0) * 1e3, O.last_phase_ms(), res

    max_threads = max(1, min(budget["affinity"] or 1, 64))
    res = None
    first_ms, first_phases, res = commit(min(max_threads, max(usable, 8)), res)   # faults the outputs in; sizes the sample
    sweep = {}
    quick = os.environ.get("WF_BENCH_CPU_QUICK") == "1"  # tests: one commitment is the sample (the root gate, not the figure, is what they check)
    if first_ms > 3000.0 or quick:  # a slow workload for the CPU (cfg 3): that commitment is the bounded sample
        best_t = min(max_threads, max(usable, 8))
        times = [(first_ms, first_phases)]
        warmups = 0
    else:
        cands = sorted({t for t in (8, 16, 32, 64, usable) if 1 <= t <= max_threads} or {max_threads})
        for t in cands:
            commit(t, res)  # threads of this count spun up
            ts = sorted(commit(t, res)[0] for _ in range(2 if first_ms > 300 else 3))
            sweep[t] = round(ts[len(ts) // 2], 2)
        best_t = min(sweep, key=sweep.get)
        for _ in range(warmups):
            commit(best_t, res)
        times = [commit(best_t, res)[:2] for _ in range(runs)]
    runs = len(times)
    times.sort(key=lambda x: x[0])
    median, phases = times[len(times) // 2]
    ms = [t for t, _ in times]
    threads = best_t
    # one thread's time per compression (the phase's wall clock x threads / compressions): comparable with the reference's
    # published single-thread 2-to-1 hash latency -- the tree phase is exactly N - 1 such hashes
    ns_tree = phases[3] * 1e6 * threads / (N - 1)
    ns_leaf = phases[2] * 1e6 * threads / leaf_comp
    # against the threads started, and against the CPUs the cgroup really grants (32 threads on a 16-CPU quota can reach 0.5 at best)
    granted = max(1, min(threads, usable))
    eff = {"merkle": round(ns_single / ns_tree, 3) if ns_tree > 0 else None,
           "hash_rows": round(ns_single / ns_leaf, 3) if ns_leaf > 0 else None,
           "merkle_vs_cpus_granted": round(ns_single / ns_tree * threads / granted, 3) if ns_tree > 0 else None,
           "hash_rows_vs_cpus_granted": round(ns_single / ns_leaf * threads / granted, 3) if ns_leaf > 0 else None,
           "cpus_granted": granted}
    # `cores` = the CPUs this run could really use (threads capped by the cgroup quota): the figure to compare across boxes;
    # `threads` = the OpenMP threads started (the best of the sweep)
    return dict(value=model["field_ops"] / (median * 1e-3), unit="field-ops/s", cores=granted, threads=threads, kind="port",
                label="C restatement of the reference's concurrent CPU path (oracle/, OpenMP; BLAKE3 compression vectorised as in the "
                      "blake3 crate's single-compression SSE form; Merkle tree by sub-trees per thread as merkle/concurrent.rs) -- not the "
                      "Rust binary, which cannot be built here",
                sample=f"{runs} full commitments ({wl['n_traces']} x 2^{wl['log_r']} x {wl['n_cols']} {wl['field']}, blowup {1 << wl['log_b']}) "
                       f"on {threads} threads after {warmups} warm-ups, outputs preallocated and first-touched by the workers; "
                       f"median {median:.0f} ms, min {ms[0]:.0f} ms",
                median_ms=median, min_ms=ms[0], max_ms=ms[-1], spread=round((ms[-1] - ms[0]) / median, 3), runs=runs, warmups=warmups,
                cpu_budget=budget, threads_usable=usable,
                thread_sweep_median_ms=sweep or None,
                phase_ms={"interpolate": round(phases[0], 2), "evaluate": round(phases[1], 2), "hash_rows": round(phases[2], 2),
                          "merkle": round(phases[3], 2)},
                ns_per_compression={"single_thread_measured_here": round(ns_single, 1), "merkle_2_to_1": round(ns_tree, 1),
                                    "leaf_rows": round(ns_leaf, 1), "threads": threads,
                                    "parallel_efficiency": eff,
                                    "reference_published_2_to_1_ns": "62-106 (single thread; /root/reference/crypto/README.md:69-75)",
                                    "note": "phase wall clock x threads / compressions: an upper bound on the per-thread cost (includes "
                                            "imbalance and memory stalls); efficiency = single-thread ns measured in this run / that; *_vs_cpus_granted rescales "
                                            "by threads / min(threads, quota) -- the quota is enforced per 100 ms period, so a phase shorter "
                                            "than that can burst above it (values > 1)"},
                cpu_model=cpu_model(), threads_pinned=os.environ.get("OMP_PROC_BIND") == "close",
                omp_places=os.environ.get("OMP_PLACES"), root=res["root"].hex(),
                root_matches_gpu=(None if gpu_root is None else res["root"].hex() == gpu_root),
                reference_toolchain={"cargo": probe(["cargo", "--version"]), "rustc": probe(["rustc", "--version"])})


def with_transfers(ctx, capi, params, trace_host, gpu_root):
    """The commitment through the entry points that take HOST columns (what Prover::build_trace_commitment hands
    over): copy-out form (64 MiB in, LDE + leaves + nodes + polys out over PCIe) and resident form (64 MiB in, the
    32-byte root out).  Median of 3 after one warm-up; outside the timed region."""
    import ctypes as C
    import numpy as np
    L = capi.load()
    cols = [np.ascontiguousarray(c) for c in trace_host]
    out = {}
    N = 1 << (LOG_R + LOG_B)
    polys = [np.zeros_like(c) for c in cols]
    lde = np.zeros((N, 8), dtype=np.uint64)
    leaves = np.zeros((N, 32), dtype=np.uint8)
    nodes = np.zeros((N, 32), dtype=np.uint8)
    root = np.zeros(32, dtype=np.uint8)
    ts = []
    for i in range(4):
        t0 = time.perf_counter()
        capi._check(L.wf_trace_commit(ctx._h, C.byref(params), capi._ptr_array(cols), capi._ptr_array(polys),
                                      capi._ptr_array([lde]), capi._p(leaves), capi._p(nodes), capi._p(root)))
        ts.append((time.perf_counter() - t0) * 1e3)
    out["host_buffers_ms"] = sorted(ts[1:])[1]
    out["host_buffers_root_matches"] = bytes(root).hex() == gpu_root
    ts = []
    for i in range(4):
        t0 = time.perf_counter()
        com, _ = ctx.trace_commit_resident(params, cols)
        ts.append((time.perf_counter() - t0) * 1e3)
        r = com.root().hex()
        com.close()
    out["resident_from_host_ms"] = sorted(ts[1:])[1]
    out["resident_root_matches"] = r == gpu_root
    # A stream of proofs: two host threads, a context each (contexts are independent), so that one proof's upload runs
    # under the other's kernels -- a single commitment cannot hide its own 64 MiB upload: every evaluation tile needs
    # the coefficients of whole columns.
    import threading

    def pipelined(columns, n_each=6):
        roots = []

        def worker():
            c2 = capi.Context(ctx.device)
            com, _ = c2.trace_commit_resident(params, columns)  # warm-up: scratch, tables
            com.close()
            barrier.wait()
            for _ in range(n_each):
                com, _ = c2.trace_commit_resident(params, columns)
                roots.append(com.root().hex())
                com.close()
            c2.close()

        barrier = threading.Barrier(3)
        th = [threading.Thread(target=worker) for _ in range(2)]
        for t in th:
            t.start()
        barrier.wait()
        t0 = time.perf_counter()
        for t in th:
            t.join()
        ms = (time.perf_counter() - t0) * 1e3 / (2 * n_each)
        return ms, all(x == gpu_root for x in roots) and len(roots) == 2 * n_each

    out["resident_pipelined_ms_per_commit"], out["resident_pipelined_roots_match"] = pipelined(cols)

    # The stream of proofs the way the library offers it (wf_trace_commit_resident_async): ONE context, the columns of
    # proof k + 1 on the copy stream under the kernels of proof k, roots through pinned slots.
    def streamed(columns, n=12, repeats=5):
        """Median and minimum ms per commitment over `repeats` batches of n (round 5: one batch was too thin a sample -- on a fresh
        box a single hiccup of ~30 ms inside the one timed batch read as 3.8 ms per commitment against 1.4 everywhere else)."""
        # warm-up at the FULL depth of a batch: with pinned columns the asynchronous call returns in 0.1 ms, so the first batch is the first
        # time ~300 operations (12 commitments x copies, kernels, events) are outstanding on the two streams together, and the runtime
        # stalls once on it -- 55 ms to 1.3 s for one commitment's wait in scripts/stream_probe.py / the round-5 record
        # (profiles/r05_stream_probe.txt); a warm-up of two commitments did not reach that depth.  Reported, not hidden: warmup_ms_per_commit.
        t0 = time.perf_counter()
        warm = ctx.trace_commit_resident_batch(params, [columns] * n)
        warm_ms = (time.perf_counter() - t0) * 1e3 / n
        for c in warm:
            c.close()
        per, ok = [], True
        for _ in range(repeats):
            t0 = time.perf_counter()
            coms = ctx.trace_commit_resident_batch(params, [columns] * n)
            per.append((time.perf_counter() - t0) * 1e3 / n)
            ok = ok and all(c.root().hex() == gpu_root for c in coms)
            for c in coms:
                c.close()
        per_sorted = sorted(per)
        return per_sorted[len(per) // 2], ok, {"min": round(per_sorted[0], 4), "max": round(per_sorted[-1], 4), "batches_in_order": [round(x, 4) for x in per],
                                               "warmup_ms_per_commit": round(warm_ms, 4)}

    out["resident_stream_ms_per_commit"], out["resident_stream_roots_match"], out["resident_stream_batches"] = streamed(cols)
    # the same with the host columns in PINNED memory (what a host gets from hipHostMalloc): asynchronous DMA
    try:
        import torch
        pinned = [torch.from_numpy(c.view(np.int64)).pin_memory().numpy().view(np.uint64) for c in cols]
        ts = []
        for i in range(4):
            t0 = time.perf_counter()
            com, _ = ctx.trace_commit_resident(params, pinned)
            ts.append((time.perf_counter() - t0) * 1e3)
            com.close()
        out["resident_from_pinned_host_ms"] = sorted(ts[1:])[1]
        out["resident_pipelined_pinned_ms_per_commit"], _ = pipelined(pinned)
        out["resident_stream_pinned_ms_per_commit"], out["resident_stream_pinned_roots_match"], out["resident_stream_pinned_batches"] = streamed(pinned)
    except Exception as e:  # noqa: BLE001 -- an optional figure
        out["resident_from_pinned_host_ms"] = f"not measured: {e}"
    # a WIDE trace (2^20 x 64: eight segments) from host columns: the upload runs segment by segment under the kernels of the
    # previous segments (the single-segment metric workload above has nothing to run it under); same call with the overlap
    # switched off for comparison
    try:
        import numpy as np
        rng = np.random.default_rng(7)
        wide = [rng.integers(0, 2**62, size=1 << LOG_R, dtype=np.uint64) for _ in range(64)]
        wp = capi.make_params(capi.F64, 1, LOG_R, LOG_B, 64, 1)

        def wide_commit():
            t0 = time.perf_counter()
            com, _ = ctx.trace_commit_resident(wp, wide)
            ms = (time.perf_counter() - t0) * 1e3
            root = com.root()
            com.close()
            return ms, root

        wide_commit()
        a = sorted(wide_commit() for _ in range(3))[1]
        # the same with the upload in front of the kernels: a second context created with WF_EXP_NO_PIPELINE set (the
        # library reads its tuning switches once, when a context is created)
        # (process environment: safe here because with_transfers runs on single-rank records only -- rank_main calls it under
        # `world == 1`, so no peer rank thread can be creating a context in this window)
        os.environ["WF_EXP_NO_PIPELINE"] = os.environ["WF_EXP_ENABLE"] = "1"
        try:
            serial_ctx = capi.Context(ctx.device)
        finally:
            del os.environ["WF_EXP_NO_PIPELINE"], os.environ["WF_EXP_ENABLE"]

        def wide_commit_serial():
            t0 = time.perf_counter()
            com, _ = serial_ctx.trace_commit_resident(wp, wide)
            ms = (time.perf_counter() - t0) * 1e3
            root = com.root()
            com.close()
            return ms, root

        wide_commit_serial()
        b = sorted(wide_commit_serial() for _ in range(3))[1]
        serial_ctx.close()
        out["wide_2p20x64_from_host_ms"] = a[0]
        out["wide_2p20x64_from_host_serial_upload_ms"] = b[0]
        out["wide_roots_match"] = a[1] == b[1]
        ctx.release_cached()
    except Exception as e:  # noqa: BLE001 -- a side measurement must not take the benchmark line down
        out["wide_error"] = f"{type(e).__name__}: {e}"
    out["note"] = ("wall clock around the C call, PCIe included; median of 3; host columns pageable numpy arrays unless 'pinned'; "
                   "pipelined = two host threads with a context each committing back to back, wall / commitments; stream = ONE context, "
                   "wf_trace_commit_resident_async (upload of proof k + 1 under the kernels of proof k), wall / commitments; wide = 2^20 x 64 "
                   "f64 (512 MiB of columns) with the upload under the kernels vs in front of them")
    return out


DUMP_SEED = 0x44554D50          # the rows sampled by --dump-outputs: fixed, so that two builds dump the same positions
DUMP_MAX_ROWS = 1 << 16
DUMP_MAX_BYTES = 12 << 20       # per array, as written (4 arrays + the root stay under 64 MB)


def dump_outputs(torch, out_dir, root, arrays):
    """--dump-outputs: write the outputs of the last timed step as out_dir/<name>.npy.  root: uint8 (32,) tensor, written
    whole.  arrays: name -> (tensor, row_elems) -- the tensor is viewed as rows of row_elems elements and a seeded sample
    of at most DUMP_MAX_ROWS rows (all of them when fewer) is written.  uint8 -> float32 bytes; int64 (u64 words) ->
    float64 pairs of 32-bit limbs (lo, hi), both exact.  The caller has synchronised the device."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "root.npy"), root.cpu().numpy().astype(np.float32))
    for i, (name, (t, row_elems)) in enumerate(sorted(arrays.items())):
        rows = t.reshape(-1, row_elems)
        limbs = t.dtype == torch.int64
        row_bytes = row_elems * (16 if limbs else 4)
        k = min(rows.shape[0], DUMP_MAX_ROWS, max(1, DUMP_MAX_BYTES // row_bytes))
        if k < rows.shape[0]:
            idx = np.sort(np.random.default_rng([DUMP_SEED, i]).choice(rows.shape[0], k, replace=False))
            rows = rows.index_select(0, torch.from_numpy(idx).to(rows.device))
        a = rows.cpu().numpy()
        if limbs:
            a = a.view(np.uint64)
            a = np.stack([a & np.uint64(0xFFFFFFFF), a >> np.uint64(32)], axis=-1).astype(np.float64)
        else:
            a = a.astype(np.float32)
        np.save(os.path.join(out_dir, name + ".npy"), a)


class TorchRcclComm:
    """Fallback collective for --mode proofs when wf_comm could not be created: torch.distributed over RCCL."""
    transport = "torch"

    def __init__(self, torch, device, reason):
        import torch.distributed as dist
        self.torch, self.dist, self.device, self.reason = torch, dist, device, reason
        dist.init_process_group("nccl", device_id=device)

    def barrier(self):
        self.dist.barrier()

    def max_f64(self, value):
        t = self.torch.tensor([value], dtype=self.torch.float64, device=self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def all_gather_tensors(self, mine, out):
        self.dist.all_gather_into_tensor(out, mine.contiguous())

    def close(self):
        self.dist.destroy_process_group()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_limited(cmd, env, limit, what):
    """Run `cmd` as a child in its own process group under a wall-clock limit, passing its stdout through line by line while
    keeping a copy.  Returns (exit code, captured stdout, captured stderr tail); 124 when the limit ended the group."""
    import signal
    import threading
    child = subprocess.Popen(cmd, env=env, start_new_session=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                             errors="replace")
    out_lines, err_lines = [], []

    def tee(src, dst, keep):
        for line in src:
            keep.append(line)
            dst.write(line)
            dst.flush()

    pumps = [threading.Thread(target=tee, args=(child.stdout, sys.stdout, out_lines), daemon=True),
             threading.Thread(target=tee, args=(child.stderr, sys.stderr, err_lines), daemon=True)]
    for t in pumps:
        t.start()
    rc = None
    try:
        rc = child.wait(timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"bench.py: {what} did not finish within {limit:.0f} s; ending the process group", file=sys.stderr, flush=True)
        for sig, grace in ((signal.SIGTERM, 10), (signal.SIGKILL, 10)):
            try:
                os.killpg(child.pid, sig)  # the group this call created (start_new_session): the launcher and its ranks
            except ProcessLookupError:
                break
            try:
                child.wait(timeout=grace)
                break
            except subprocess.TimeoutExpired:
                continue
        rc = 124
    for t in pumps:
        t.join(timeout=5)
    return rc, "".join(out_lines), "".join(err_lines[-200:])


def launch_ranks(n):
    """`python bench.py --gpus N` as a plain command: start one rank per GPU and get out of the way.  This process has
    not imported torch or touched the GPU; the ranks are children, not an exec of this process.  The children run in
    their own process group under a wall-clock limit (WF_BENCH_LAUNCH_TIMEOUT_S, default 900 s): on expiry exactly that
    group is ended and this process exits non-zero -- a rank stuck in a collective cannot hang the caller.

    Fallback (round 5): if the process launcher fails WITHOUT a benchmark line -- and not through a parity gate and not at the
    limit: e.g. a box that allows fewer processes on a card than the launcher needs -- a FRESH child runs the same command
    with `--ranks threads` (one process, one host thread per GPU, the same RCCL communicator, steps and gates).  The child's
    record says in `collective.ranks` that the fallback ran and why.  WF_BENCH_NO_FALLBACK=1 turns it off."""
    launcher = os.environ.get("WF_BENCH_LAUNCHER")  # test hook: a stand-in for `python -m torch.distributed.run`
    head = launcher.split() if launcher else [sys.executable, "-m", "torch.distributed.run"]
    cmd = head + ["--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
                  os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL between processes needs it on this host driver
    env.setdefault("OMP_NUM_THREADS", "8")
    limit = float(os.environ.get("WF_BENCH_LAUNCH_TIMEOUT_S", "900"))
    t0 = time.monotonic()
    rc, out, err = _run_limited(cmd, env, limit, f"the {n} ranks")
    has_line = any(l.startswith("{") for l in out.splitlines())
    parity = "PARITY FAILURE" in out or "PARITY FAILURE" in err
    if rc == 0 or has_line or parity or rc == 124 or os.environ.get("WF_BENCH_NO_FALLBACK") == "1":
        return rc
    left = limit - (time.monotonic() - t0)
    if left < 30:
        return rc
    last = [l.strip() for l in err.splitlines() if l.strip()]
    reason = f"process launcher exited {rc} without a benchmark line" + (f" (last stderr line: {last[-1][:160]})" if last else "")
    print(f"bench.py: {reason}; starting a fresh child with --ranks threads", file=sys.stderr, flush=True)
    argv = [a for a in sys.argv[1:]]
    if "--ranks" in argv:  # (only reached when --ranks processes was given explicitly)
        i = argv.index("--ranks")
        del argv[i:i + 2]
    env2 = dict(env)
    env2["WF_BENCH_FALLBACK_REASON"] = reason
    rc2, _, _ = _run_limited([sys.executable, os.path.abspath(__file__)] + argv + ["--ranks", "threads"], env2, left,
                             f"the {n} rank threads (fallback)")
    return rc2


def verify_multi_rank(torch, capi, shard, ctx, comm, args, packed, params, rank, world, device, stream, trace, roots, all_roots, top,
                      bufs):
    """Parity gates of a multi-rank run, outside the timed region.  Collective: every rank calls it.
      proofs : the gathered roots must be, for every rank r and timed step k, the root of rank r's proof -- rank 0 commits
               each rank's trace (same seed) once more on its own GPU through the single-GPU entry point (itself checked
               against the CPU oracle by the N = 1 run and the parity tests) and compares; every rank also checks that
               its own slice of the gathered array is what it sent.
      packed : rank 0 commits the same packed traces unsharded (wf_trace_commit_dev) and compares the root with the
               sharded one; the roots of all ranks are gathered and must be identical.
    Returns (ok, details); the verdict is agreed over all ranks (max), so that every rank exits with the same code."""
    n_steps = args.steps
    bad = []
    R, N = 1 << LOG_R, 1 << (LOG_R + LOG_B)
    torch.cuda.synchronize()
    if not packed:
        got = all_roots[:world * n_steps].cpu().numpy().reshape(world, n_steps, 32)
        mine = roots[:n_steps].cpu().numpy()
        if not (got[rank] == mine).all():
            bad.append(f"rank {rank}: its slice of the gathered roots differs from the roots it sent")
        if rank == 0:
            polys, lde, leaves, nodes = bufs
            for r in range(world):
                pid = shard.proofs_of_rank(world, r, world)[0]
                t = trace if r == 0 else rand_f64_dev(torch, N_COLS * R, shard.seed_of_proof(0x57415446, pid), device)
                torch.cuda.synchronize()  # (the generator ran on torch's default stream, the commitment runs on `stream`)
                with torch.cuda.stream(stream):
                    ctx.trace_commit_dev(params, t.data_ptr(), polys.data_ptr(), lde.data_ptr(), leaves.data_ptr(),
                                         nodes.data_ptr(), stream.cuda_stream)
                    torch.cuda.synchronize()
                want = nodes[1].cpu().numpy()
                wrong = [k for k in range(n_steps) if not (got[r, k] == want).all()]
                if wrong:
                    bad.append(f"rank {r}: gathered root of step(s) {wrong[:4]} != root of its proof recomputed on rank 0 "
                               f"({bytes(got[r, wrong[0]]).hex()[:16]} vs {bytes(want).hex()[:16]})")
        what = f"{world} x {n_steps} gathered roots == each rank's proof re-committed on rank 0"
    else:
        my_root = top[1:2].contiguous()
        every = torch.zeros((world, 32), dtype=torch.uint8, device=device)
        with torch.cuda.stream(stream):
            comm.all_gather_roots(my_root.data_ptr(), 1, every.data_ptr(), stream.cuda_stream)
            comm.stream_wait(stream.cuda_stream)
        ev = every.cpu().numpy()
        if not (ev == ev[rank]).all():
            bad.append(f"rank {rank}: the ranks hold different roots of the one packed commitment")
        if rank == 0:
            n_traces = PACKED_TRACES
            full_lde = torch.empty(n_traces * N * 8, dtype=torch.int64, device=device)
            full_leaves = torch.empty((N, 32), dtype=torch.uint8, device=device)
            full_nodes = torch.empty((N, 32), dtype=torch.uint8, device=device)
            polys = bufs[0]
            with torch.cuda.stream(stream):
                ctx.trace_commit_dev(params, trace.data_ptr(), polys.data_ptr(), full_lde.data_ptr(), full_leaves.data_ptr(),
                                     full_nodes.data_ptr(), stream.cuda_stream)
                torch.cuda.synchronize()
            want = full_nodes[1].cpu().numpy()
            if not (ev[0] == want).all():
                bad.append(f"sharded root {bytes(ev[0]).hex()[:16]} != unsharded commitment of the same traces {bytes(want).hex()[:16]}")
            del full_lde, full_leaves, full_nodes
        what = f"sharded root on all {world} ranks == unsharded wf_trace_commit_dev of the same traces on rank 0"
    for line in bad:
        print("PARITY FAILURE:", line, file=sys.stderr, flush=True)
    failed = comm.max_f64(1.0 if bad else 0.0) > 0.0
    return (not failed), {"checked": what, "ok": not failed}


class ThreadRanks:
    """What the ranks of --ranks threads share: the RCCL unique id (drawn once, before the threads start) or the in-process
    rehearsal transport, and a barrier for the few host-side hand-overs."""

    def __init__(self, world, backend):
        import threading
        from starkpack_winterfell_amd import shard
        self.world, self.backend = world, backend
        self.uid = shard.unique_id() if backend == "rccl" else None
        self.loopback = shard.Loopback(world, timeout=float(os.environ.get("WF_COMM_TIMEOUT_S", "300"))) if backend == "loopback" else None
        self.failed = threading.Event()  # a rank failed: its peers are released (loopback) or given a short grace (RCCL)
        self.rc = [None] * world

    def abort(self):
        self.failed.set()
        if self.loopback is not None:
            try:
                self.loopback.barrier.abort()  # peers waiting in a rehearsal collective raise BrokenBarrierError
            except Exception:  # noqa: BLE001
                pass


def run_threads(args):
    """`python bench.py --gpus N --ranks threads`: the N ranks as N host threads of THIS process, one GPU each (device r for
    rank r; `r % device_count` only under the loopback rehearsal).  Returns the exit code: non-zero if any rank failed, 124
    if the ranks did not finish within WF_BENCH_LAUNCH_TIMEOUT_S (the process then ends without joining them)."""
    import threading
    import traceback
    n = args.gpus
    backend = os.environ.get("WF_BENCH_BACKEND", "rccl")
    if backend == "gloo":
        backend = "loopback"  # (the process-group rehearsal has no meaning inside one process)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch  # noqa: F401  (first import on the main thread)
    import starkpack_winterfell_amd.capi as capi
    n_dev = capi.device_count()
    if n_dev < 1:
        print("bench.py: no HIP device", file=sys.stderr, flush=True)
        return 1
    if backend == "rccl" and n_dev < n:
        print(f"bench.py: --ranks threads on RCCL needs one device per rank ({n_dev} device(s), {n} ranks); "
              f"WF_BENCH_BACKEND=loopback rehearses the same control flow on fewer", file=sys.stderr, flush=True)
        return 1
    shared = ThreadRanks(n, backend)

    def body(r):
        try:
            rank_main(args, r, n, r, "threads", shared)
            shared.rc[r] = 0
        except SystemExit as e:
            if e.code not in (None, 0):
                print(f"rank {r}: {e.code}", file=sys.stderr, flush=True)
                shared.abort()  # (a parity gate exits this way: the peers must not sit in their next collective)
            shared.rc[r] = 0 if e.code in (None, 0) else 1
        except BaseException:  # noqa: BLE001 -- a rank's failure is the run's failure
            traceback.print_exc()
            shared.rc[r] = 1
            shared.abort()

    threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(n)]
    for t in threads:
        t.start()
    limit = float(os.environ.get("WF_BENCH_LAUNCH_TIMEOUT_S", "900"))
    deadline = time.monotonic() + limit
    grace = float(os.environ.get("WF_BENCH_PEER_GRACE_S", "20"))
    while any(t.is_alive() for t in threads) and time.monotonic() < deadline:
        threads[0].join(timeout=0.2) if threads[0].is_alive() else time.sleep(0.2)
        if shared.failed.is_set():  # a rank failed: peers inside an RCCL collective get a short grace, not the whole limit
            end = time.monotonic() + grace
            while any(t.is_alive() for t in threads) and time.monotonic() < end:
                time.sleep(0.2)
            if any(t.is_alive() for t in threads):
                print(f"bench.py: a rank failed and its peers did not return within {grace:.0f} s; ending the process", file=sys.stderr, flush=True)
                sys.stdout.flush()
                os._exit(1)
            break
    if any(t.is_alive() for t in threads):
        print(f"bench.py: the {n} rank threads did not finish within {limit:.0f} s; ending the process", file=sys.stderr, flush=True)
        sys.stdout.flush()
        os._exit(124)  # the stuck threads sit inside the runtime: no orderly shutdown to wait for
    return 0 if all(rc == 0 for rc in shared.rc) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", choices=("proofs", "packed"), default="proofs")
    ap.add_argument("--ranks", choices=("processes", "threads"), default=os.environ.get("WF_BENCH_RANKS", "processes"),
                    help="N > 1: one process per GPU under torch.distributed.run (default), or one host thread per GPU in this "
                         "process -- both on RCCL inside libwf_lde.so, same steps, gates and JSON line")
    ap.add_argument("--config", choices=tuple(CONFIGS), default="cfg2",
                    help="workload (single GPU for all but cfg2): cfg2 = the metric; cfg3 = 2^22 x 64 f64; cfg5 = f128 2^18 x 10; "
                         "dowork = the reference's example defaults (512 packed f128 traces of 2^10)")
    ap.add_argument("--full", action="store_true",
                    help="the whole record: in-run ALU yardstick, transfers, CPU baseline; admits --config and --per-launch")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the last step as DIR/<name>.npy (rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) leave the CPU baseline out")
    ap.add_argument("--no-transfers", action="store_true", help="(--full) leave with_transfers out")
    ap.add_argument("--per-launch", action="store_true", help="(--full) also report HIP-event times of every kernel launch")
    ap.add_argument("--inject-fault", choices=("root", "hang"), default=None,
                    help="test hook (tests/test_gpu_multi_device.py), applied AFTER the timed region: 'root' flips a byte of a "
                         "root on rank 1 so that the parity gate must fire; 'hang' makes rank 1 sleep so that the launcher's limit must")
    args = ap.parse_args()

    if args.steps < 1 or args.warmup < 0:
        sys.exit("--steps must be >= 1 and --warmup >= 0")
    if not args.full and (args.config != "cfg2" or args.per_launch):
        sys.exit("--config other than cfg2 and --per-launch belong to the full record: add --full")
    if args.config != "cfg2" and (args.gpus > 1 or args.mode != "proofs"):
        sys.exit("--config other than cfg2 is a single-GPU record of the default mode (the multi-GPU modes run the metric's workload)")
    # N > 1 as a plain command: the route is chosen HERE, before this process has touched the GPU -- child processes (never
    # an exec of this one), or threads of this process
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(run_threads(args) if args.ranks == "threads" else launch_ranks(args.gpus))
    rank_main(args, int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0")),
              "processes", None)


def rank_main(args, rank, world, local_rank, route, shared):
    """One rank: a process started by torch.distributed.run (route "processes"; also the single-GPU run) or a thread of
    run_threads (route "threads")."""
    import copy
    args = copy.copy(args)  # (per rank: args.gpus is overwritten below)
    import torch
    import starkpack_winterfell_amd.capi as capi
    from starkpack_winterfell_amd import shard

    args.gpus = world
    # one rank per GPU; the modulo only matters for rehearsals of the multi-rank control flow on a box with fewer GPUs
    # than ranks (WF_BENCH_BACKEND=gloo) -- RCCL itself refuses two ranks on one device
    dev_index = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    backend = os.environ.get("WF_BENCH_BACKEND", "rccl")

    ctx = capi.Context(dev_index)
    comm = None
    if world > 1 and route == "threads":
        # one communicator per thread, all from the id the parent drew: ncclCommInitRank returns when all `world` threads
        # have called it (or the rehearsal transport: the same partitioning and kernels, bytes through host memory)
        if shared.backend == "loopback":
            comm = shard.Comm.with_transport(ctx, rank, world, *shared.loopback.collectives(rank))
        else:
            comm = shard.Comm.with_unique_id(ctx, shared.uid, rank, world)
    elif world > 1:
        if backend == "gloo":
            import torch.distributed as dist
            dist.init_process_group("gloo")
            comm = shard.Comm.with_process_group(ctx)
        else:
            # RCCL inside libwf_lde.so (wf_comm).  The ranks agree through the store on whether every one of them got its
            # communicator; if not (nothing like that has been seen, but this path cannot be rehearsed with N > 1 on the
            # one-GPU boxes it was built on) the roots travel through torch.distributed's RCCL binding instead and the
            # JSON line says so -- a measured run with the fallback named beats no run.
            store = shard.store_from_env(rank, world)
            err = ""
            try:
                comm = shard.Comm.with_store(ctx, store, rank, world)
            except Exception as e:  # noqa: BLE001 -- reported in the JSON line
                err = f"{type(e).__name__}: {e}"
            store.set(f"wf_comm_status_{rank}", err.encode() or b"ok")
            status = [bytes(store.get(f"wf_comm_status_{r}")).decode() for r in range(world)]
            if any(x != "ok" for x in status):
                if comm is not None:
                    comm.close()
                if args.mode == "packed":
                    raise SystemExit("wf_comm could not be created on every rank: " + "; ".join(status))
                comm = TorchRcclComm(torch, device, next(x for x in status if x != "ok"))

    packed = args.mode == "packed"
    wl = dict(CONFIGS[args.config])
    if packed:
        wl["n_traces"] = PACKED_TRACES
    n_traces, n_cols, log_r, log_b = wl["n_traces"], wl["n_cols"], wl["log_r"], wl["log_b"]
    is64 = wl["field"] == "f64"
    elem_bytes, words = (8, 1) if is64 else (16, 2)
    model = work_model(log_r, log_b, n_cols, elem_bytes, n_traces)
    params = capi.make_params(capi.F64 if is64 else capi.F128, 1, log_r, log_b, n_cols, n_traces)
    R, N = 1 << log_r, 1 << (log_r + log_b)
    row_width = 8 * ((n_cols + 7) // 8)
    # packed: every rank holds the same traces (one proof); proofs: a trace of its own per rank
    proof_id = 0 if packed else shard.proofs_of_rank(world, rank, world)[0]
    seed = shard.seed_of_proof(0x57415446, proof_id)
    trace = (rand_f64_dev if is64 else rand_f128_dev)(torch, n_traces * n_cols * R, seed, device)
    polys = torch.empty_like(trace)
    share = world if packed else 1  # a rank's part of the LDE rows and of the tree
    lde = torch.empty(n_traces * (N // share) * row_width * words, dtype=torch.int64, device=device)
    leaves = torch.empty((N // share, 32), dtype=torch.uint8, device=device)
    nodes = torch.empty((N // share, 32), dtype=torch.uint8, device=device)
    top = torch.zeros((2 * world, 32), dtype=torch.uint8, device=device)

    stream = torch.cuda.Stream(device=device)
    torch.cuda.synchronize()
    # --full: the driver's clock reading and the yardstick of the `alu` object, measured in THIS run on THIS GPU, before
    # the timed region
    clock_files = gpu_clock_files(torch, dev_index) if rank == 0 and args.full else []
    yard = yardstick(torch, dev_index, clock_files, CONFIGS[args.config]['field'] == 'f64') if rank == 0 and args.full else None
    ctx.profile_enable(1)  # HIP events at the logical-kernel boundaries of every timed step (5 per step, ~1 %)
    per_launch = {}

    # the roots of the K timed commitments of this rank; ranks run free of each other (independent proofs, no data-path
    # collective) and exchange all their roots once, inside the timed region: the path's single exchange
    n_keep = max(args.steps, args.warmup, 1)
    roots = torch.zeros((n_keep, 32), dtype=torch.uint8, device=device)
    all_roots = torch.zeros((world * n_keep, 32), dtype=torch.uint8, device=device)

    def step(k):
        if packed and comm is not None:
            comm.trace_commit_sharded_dev(params, trace.data_ptr(), polys.data_ptr(), lde.data_ptr(), leaves.data_ptr(),
                                          nodes.data_ptr(), top.data_ptr(), stream.cuda_stream)
            roots[k].copy_(top[1], non_blocking=True)
        else:
            ctx.trace_commit_dev(params, trace.data_ptr(), polys.data_ptr(), lde.data_ptr(), leaves.data_ptr(),
                                 nodes.data_ptr(), stream.cuda_stream)
            roots[k].copy_(nodes[1], non_blocking=True)

    def gather(k):
        if comm is not None and not packed:
            if comm.transport == "torch":
                comm.all_gather_tensors(roots[:k], all_roots[:world * k])
            else:
                comm.all_gather_roots(roots.data_ptr(), k, all_roots.data_ptr(), stream.cuda_stream)

    with torch.cuda.stream(stream):
        for k in range(args.warmup):
            step(k)
        gather(max(args.warmup, 1))  # warm the communicator up as well
        torch.cuda.synchronize()
        ctx.profile_read()  # drop the warm-up events
        if comm is not None:
            comm.barrier()
        torch.cuda.synchronize()
        sampler = ClockSampler(clock_files)
        sampler.__enter__()  # the driver's clock reading while the timed steps run (a reader thread; no GPU work)
        t0 = time.perf_counter()
        for k in range(args.steps):
            step(k)
        gather(args.steps)
        if comm is not None and comm.transport != "torch":
            comm.stream_wait(stream.cuda_stream)  # the same wait under wf_comm's watchdog: an error, not a hang, if a peer died
        torch.cuda.synchronize()
        if comm is not None:
            comm.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        sampler.__exit__()
        # HIP events recorded on the launch stream in front of every kernel of the K timed steps
        for name, ms in ctx.profile_read():
            per_launch.setdefault(name, []).append(ms)

    if args.dump_outputs and rank == 0:
        # the buffers still hold the last timed step's results (nothing above writes them); the gates below reuse them
        outs = {"polys": (polys, words), "lde": (lde, row_width * words), "leaves": (leaves, 32), "nodes": (nodes, 32)}
        if packed and comm is not None:
            outs["top"] = (top, 32)
        dump_outputs(torch, args.dump_outputs, roots[args.steps - 1], outs)

    per_rank_ms, comm_info = None, None
    if comm is not None:
        if comm.transport != "torch":
            # every rank's own time for its K steps, and what the transport says about the communicator each rank holds
            per_rank_ms = [t / args.steps * 1e3 for t in comm.gather_f64(elapsed)]
            mine = comm.info()
            comm_info = {"transport": mine["transport"], "count": mine["count"],
                         "user_ranks": [int(x) for x in comm.gather_f64(mine["user_rank"])],
                         "devices": [int(x) for x in comm.gather_f64(mine["device"])],
                         "counts": [int(x) for x in comm.gather_f64(mine["count"])]}
        elapsed = comm.max_f64(elapsed)  # MAX over ranks
    verified = None
    if args.inject_fault == "hang" and rank == world - 1 and world > 1:
        time.sleep(3600)  # (threads route: a daemon thread -- the parent's limit ends the process)
    if args.inject_fault == "root" and world > 1:
        torch.cuda.synchronize()
        if packed and rank == world - 1:
            top[1, 0] ^= 1                                  # the last rank's copy of the packed commitment's root
        if not packed and rank == 0:
            all_roots[(world - 1) * args.steps, 0] ^= 1     # what rank 0 received as the last rank's first root
        torch.cuda.synchronize()
    if comm is not None:
        # a multi-rank number is only printed for results that are right: root parity gates, outside the timed region
        ok, verified = verify_multi_rank(torch, capi, shard, ctx, comm, args, packed, params, rank, world, device, stream, trace,
                                         roots, all_roots, top, (polys, lde, leaves, nodes))
        if not ok:
            comm.close()
            ctx.close()
            raise SystemExit("PARITY FAILURE in the multi-rank run (see stderr): no benchmark line is printed")
    root_hex = bytes(roots[args.steps - 1].cpu().numpy()).hex()
    n_roots = world * args.steps if (comm is not None and not packed) else args.steps

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        commits = (1 if packed else world) * args.steps
        value = commits * model["field_ops"] / elapsed
        avg = {k: sum(v) / len(v) for k, v in per_launch.items()}
        logical = {
            "interpolate": sum(v for k, v in avg.items() if k.startswith(("interpolate", "layout"))),
            "evaluate": sum(v for k, v in avg.items() if k.startswith("evaluate")),
            "hash_rows": avg.get("hash_rows", 0.0),
            "merkle": avg.get("merkle", 0.0),
        }
        if args.per_launch:  # a separate, finer pass outside the timed region: one event per kernel launch
            ctx.profile_enable(2)
            with torch.cuda.stream(stream):
                for k in range(args.steps):
                    step(k)
                torch.cuda.synchronize()
            fine = {}
            for name, ms in ctx.profile_read():
                fine.setdefault(name, []).append(ms)
            avg = {k: sum(v) / len(v) for k, v in fine.items()}
        # the leaves are hashed by the last evaluation pass itself (no k_hash_rows launch, the LDE is not read back);
        # the evaluate kernel then also owns the write of the leaves
        per_rank = world if packed else 1
        bytes_k = {k: v // per_rank for k, v in model["bytes_per_kernel"].items()}
        fused_hash = "hash_rows" not in avg
        if fused_hash:
            bytes_k["evaluate"] += N * 32 // per_rank
            bytes_k["hash_rows"] = 0
        dom = max(logical, key=logical.get)
        dom_ms = logical[dom]
        achieved = bytes_k[dom] / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0
        # HBM-side bytes of the dominant kernel from the PMC passes of scripts/profile_round.sh -- quoted only while the
        # kernel sources are the ones they were measured on
        traffic, traffic_sha, traffic_rule = None, None, None
        tpath = os.path.join(ROOT, "profiles", "traffic.json" if args.config == "cfg2" else f"traffic_{args.config}.json")
        if os.path.exists(tpath) and not packed and world == 1:
            try:
                tj = json.load(open(tpath))
                traffic_sha = tj.get("_csrc_sha")
                traffic_rule = tj.get("_rule", "2 (round 4): FETCH_SIZE x 2 except k_merkle_level2")
                if traffic_sha == csrc_sha():
                    traffic = tj.get(dom, {}).get("hbm_bytes_per_step")
            except Exception:
                traffic = None
        workload = (f"{PACKED_TRACES} packed traces of 2^20 rows x 8 cols f64 under ONE tree (STARKPack), blowup 8, sharded "
                    f"by coset over {world} GPU(s)" if packed else
                    wl["label"] + "; one independent commitment per GPU per step"
                    + (", the roots of all steps all-gathered over RCCL once per run (configs[3])" if world > 1 else ""))
        # `alu`: the step against the time its butterflies and compressions take at the rates the same instruction
        # sequences reach in isolation -- measured in this run (yardstick above), with the clocks both ran at
        alu = {"butterflies": model["butterflies"], "blake3_compressions": model["compressions"]}
        if yard and "error" not in yard:
            b_rate, c_rate = yard["butterflies"]["per_s"], yard["blake3_compressions"]["per_s"]
            ideal = (model["butterflies"] / b_rate + model["compressions"] / c_rate) * 1e3 / (world if packed else 1)
            alu.update({"yardstick_butterflies_per_s": b_rate, "yardstick_compressions_per_s": c_rate,
                        "rates": "measured in this run before the timed region (csrc/yardstick.hip: register-only loops of the kernels' own "
                                 "device functions, 8 waves per SIMD; " + ("Goldilocks" if is64 else "f128") + " butterflies)",
                        "clock_mhz_driver_reading": {"yardstick_butterflies": yard["butterflies"]["clock_driver"],
                                                     "yardstick_compressions": yard["blake3_compressions"]["clock_driver"],
                                                     "timed_steps": sampler.summary(),
                                                     "source": "hwmon freq1_input (sclk) of this GPU, read in a loop by a host thread"},
                        "ideal_ms": ideal, "frac": ideal / ms_per_step})
        elif yard is None:
            alu["not_measured"] = "the in-run yardstick is part of the full record (--full)"
        else:
            alu["error"] = yard.get("error", "not measured")
        out = {
            "metric": ("trace-LDE + Merkle-commit field-ops/s (wall-clock ms in ms_per_step), 2^20x8 f64 trace blowup=8" if args.config == "cfg2"
                       else f"trace-LDE + Merkle-commit field-ops/s (wall-clock ms in ms_per_step), {args.config} (not the headline metric)"),
            "value": value,
            "unit": "field-ops/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong" if packed else "weak",
            "vs_baseline": None,
            "dtype": ("u64 (Goldilocks, Montgomery form)" if is64 else "u128 (p = 2^128 - 45 * 2^40 + 1, canonical; 32-bit limbs)") + " + u32 (BLAKE3)",
            "data": "synthetic (seeded uniform field elements, resident in HBM)",
            "config": {"workload": workload, "name": args.config, "mode": args.mode, "field": wl["field"], "log2_trace_len": log_r,
                       "n_cols": n_cols, "blowup": 1 << log_b, "n_traces": n_traces},
            "commits_per_s": commits / elapsed,
            "collective": (None if comm is None else
                           {"transport": "RCCL inside libwf_lde.so (wf_comm, C ABI)" if comm.transport == "rccl"
                            else ("FALLBACK: torch.distributed nccl (= RCCL), wf_comm failed: " + comm.reason) if comm.transport == "torch"
                            else "wf_transport through host memory between the threads of one process (rehearsal)" if route == "threads"
                            else "wf_transport over torch.distributed gloo (rehearsal)",
                            "ranks": (("one host thread per GPU in one process" if route == "threads" else "one process per GPU (torch.distributed.run)") +
                                      (" -- FALLBACK: " + os.environ["WF_BENCH_FALLBACK_REASON"] if os.environ.get("WF_BENCH_FALLBACK_REASON") else "")),
                            # ncclCommCount / ncclCommUserRank / ncclCommCuDevice as every rank's communicator reports them
                            # (wf_comm_info): RCCL itself saying that it spans `world` ranks on `world` distinct devices
                            "nccl_comm_count": comm_info["count"] if comm_info else None,
                            "nccl_comm_counts": comm_info["counts"] if comm_info else None,
                            "nccl_user_ranks": comm_info["user_ranks"] if comm_info else None,
                            "nccl_devices": comm_info["devices"] if comm_info else None,
                            "ms_per_step_per_rank": [round(x, 4) for x in per_rank_ms] if per_rank_ms else None,
                            "rccl_version": capi.load().wf_comm_rccl_version() if comm.transport == "rccl" else None,
                            "rccl_path": (capi.load().wf_comm_rccl_path() or b"").decode() if comm.transport == "rccl" else None,
                            "verified": verified,
                            "calls": "all-to-all of leaf digests + all-gather of sub-roots per step" if packed
                            else "one all-gather of roots per run"}),
            "alu": alu,
            "path": {"b_alg_bytes": model["b_alg"], "hbm_frac": model["b_alg"] / per_rank / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                     "field_ops": model["field_ops"], "blake3_compressions": model["compressions"]},
            "roofline": {"bound": "hbm", "kernel": dom + (" (leaf hashing fused into its last pass)" if fused_hash and dom == "evaluate" else ""),
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "traffic_measured_on_csrc": traffic_sha, "traffic_rule": traffic_rule, "csrc": csrc_sha(),
                         "algorithmic_bytes": bytes_k[dom], "avg_ms": dom_ms},
            "launch_ms": {k: round(v, 4) for k, v in avg.items()},
            "root": root_hex,
            "roots_gathered": n_roots,
        }
        if world == 1 and not packed and args.full:
            th = trace.cpu().numpy().view("uint64")
            th = th.reshape(n_traces, n_cols, R) if is64 else th.reshape(n_traces, n_cols, R, 2)
            # the two side measurements must not cost the line its timed result: a failure in them is reported in place
            if not args.no_transfers and args.config == "cfg2":
                try:
                    out["with_transfers"] = with_transfers(ctx, capi, params, th[0], root_hex)
                except Exception as e:  # noqa: BLE001
                    out["with_transfers"] = {"error": f"{type(e).__name__}: {e}"}
            if not args.no_cpu_baseline:
                big = model["butterflies"] > 4e9   # cfg 3: ~15 s of 64 cores per commitment -- one run is the bounded sample
                try:
                    out["cpu_baseline"] = cpu_baseline(model, wl, [list(t) for t in th], root_hex, runs=1 if big else 5,
                                                       warmups=0 if big else 2)
                except Exception as e:  # noqa: BLE001
                    out["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}", "kind": "port"}
                if out["cpu_baseline"].get("root_matches_gpu") is False:
                    raise SystemExit("PARITY FAILURE: CPU oracle root != GPU root on the bench workload")
                if "value" in out["cpu_baseline"]:
                    out["gpu_over_cpu"] = value / out["cpu_baseline"]["value"]
        print(json.dumps(out), flush=True)
    if comm is not None:
        comm.barrier()
        comm.close()
        if backend == "gloo" and route == "processes":
            import torch.distributed as dist
            dist.destroy_process_group()
    ctx.close()


if __name__ == "__main__":
    main()
