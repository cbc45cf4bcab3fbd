"""GPU: sanity of the box's RCCL through torch.distributed ("nccl" backend, a world of one) next to the library's own
RCCL binding (tests/test_gpu_comm.py), and bench.py's line contract."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SCRIPT = r"""
import os, sys, torch, torch.distributed as dist
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=dev)
x = torch.arange(3 * 32, dtype=torch.uint8, device=dev).reshape(3, 32)
out = torch.empty((3, 32), dtype=torch.uint8, device=dev)
dist.all_gather_into_tensor(out, x)
assert torch.equal(out, x)
t = torch.tensor([1.5], dtype=torch.float64, device=dev)
dist.all_reduce(t, op=dist.ReduceOp.MAX)
dist.barrier()
dist.destroy_process_group()
print("RCCL OK")
"""


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _env():
    env = dict(os.environ)
    env.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(_free_port()), "RANK": "0", "LOCAL_RANK": "0",
                "WORLD_SIZE": "1", "WF_ROOT": ROOT, "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    return env


def test_rccl_world_of_one(capi):
    capi.load()
    out = subprocess.run([sys.executable, "-c", SCRIPT], env=_env(), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "RCCL OK" in out.stdout


def _bench_dump(out_dir, *extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra, "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    return j, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_bench_line_contract(capi, tmp_path):
    """bench.py prints one JSON line carrying the contract's keys (short plain run: no CPU baseline, no side measurements)
    and --dump-outputs writes the last step's outputs, the root among them."""
    capi.load()
    j, arrays = _bench_dump(tmp_path, "--steps", "3", "--warmup", "1", "--no-cpu-baseline")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 3 and j["roofline"]["bound"] == "hbm" and 0 < j["roofline"]["frac"] < 1
    assert j["roots_gathered"] == 3
    assert "cpu_baseline" not in j and "with_transfers" not in j          # --full only
    assert set(arrays) == {"root", "polys", "lde", "leaves", "nodes"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert bytes(arrays["root"].astype(np.uint8)).hex() == j["root"]
    assert arrays["lde"].shape[1:] == (8, 2) and arrays["lde"].max() < 2**32


def test_bench_dump_outputs_repeat(capi, tmp_path):
    """Two plain runs with the same arguments dump identical outputs (seeded inputs, fixed sample)."""
    capi.load()
    j1, a1 = _bench_dump(tmp_path / "a", "--steps", "2", "--warmup", "1")
    j2, a2 = _bench_dump(tmp_path / "b", "--steps", "2", "--warmup", "1")
    assert j1["root"] == j2["root"]
    assert set(a1) == set(a2)
    for name in a1:
        assert np.array_equal(a1[name], a2[name]), name


@pytest.mark.parametrize("config", ["cfg5", "dowork"])
def test_bench_other_configs_print_the_same_line(capi, config):
    """bench.py --full --config: the f128 workloads print the contract's line with in-run `alu` rates and pass their CPU-oracle
    root gate (cfg3 -- 2^22 x 64 -- runs the same code at a size kept for the profiling scripts)."""
    capi.load()
    env = dict(os.environ)
    env["WF_BENCH_CPU_QUICK"] = "1"  # one CPU commitment (the root gate below needs no thread sweep: it took 47 s of the suite for dowork)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--config", config, "--steps", "2", "--warmup", "1"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert j["config"]["name"] == config and j["config"]["field"] == "f128"
    assert j["roofline"]["bound"] == "hbm" and 0 < j["roofline"]["frac"] < 1
    assert j["alu"]["yardstick_butterflies_per_s"] > 1e10 and 0 < j["alu"]["frac"] < 1.5
    assert j["cpu_baseline"]["root_matches_gpu"] is True
    assert set(j["cpu_baseline"]["phase_ms"]) == {"interpolate", "evaluate", "hash_rows", "merkle"}
