"""GPU: rehearsal of the multi-process bench path the driver launches for N > 1
(`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...`).  A 1-GPU box cannot
run RCCL with two ranks on one device, so the two ranks share the device and talk over gloo
(MGN_DIST_BACKEND / MGN_SHARE_GPU, graph_physics_amd/distributed.py): same code path for parameter
broadcast, gradient all-reduce, the max-over-ranks timing and the rank-0-only sections (kernel
timing must not enter a collective), and the partitioned large-mesh record (`c4`) on a small mesh."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_bench_line():
    env = dict(os.environ, MGN_DIST_BACKEND="gloo", MGN_SHARE_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--batch", "2", "--nodes", "400", "--rounds", "3", "--rollout-steps", "2", "--full", "--no-cpu-baseline",
           "--c4-nodes", "30000", "--c4-steps", "2", "--c5-nodes", "4000"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 prints ONE line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["value"] > 0 and d["scaling"] == "weak"
    assert d["config"]["parallelism"] == "dp2" and d["config"]["global_batch_meshes"] == 4
    assert "roofline" in d and d["roofline"]["bound"] == "hbm"
    # the configs[3]-style record under the same launch: N-way node partition + halo exchange per round
    c4 = d["c4"]
    assert "2-way node partition" in c4["parallelism"] and c4["ghost_rows"] > 0 and 0 < c4["owned_nodes"] < 30000
    assert c4["train_ms_per_step"] > 0 and c4["rollout_ms_per_step"] > 0 and c4["node_train_steps_per_s"] > 0
    # one rank built the mesh and the partition, the other received them; the step's communication is timed on its own
    assert c4["mesh_build_and_partition_s_rank0"] > 0 and c4["halo_ms_per_step"] > 0 and c4["allreduce_ms_per_step"] > 0
    # configs[4] under the N > 1 launch: bf16 replicas of the Transformer
    c5 = d["c5"]
    assert c5["parallelism"].startswith("dp2") and c5["train_ms_per_step"] > 0 and "bf16" in c5["dtype"]
    assert d["step_floor"]["step_floor_ms"] > 0 and 0 < d["step_floor"]["frac_of_floor"] < 1


def test_gpus_flag_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no torch.distributed environment launches the two ranks itself and relays
    rank 0's line (round-1 advisor finding: the flag used to be parsed and ignored)."""
    env = dict(os.environ, MGN_DIST_BACKEND="gloo", MGN_SHARE_GPU="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "1", "--nodes", "300",
           "--rounds", "2", "--rollout-steps", "2", "--no-cpu-baseline", "--no-c4", "--no-kernel-timing"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 2
