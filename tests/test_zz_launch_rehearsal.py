"""Dress rehearsal of the driver's multi-GPU launch on the 1-GPU box (round-5 verdict item 3): the scaling run is one shot on hardware
the builder never sees, so its launch path — `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N`,
N processes, LPT shards of ONE batch (configs[3]), per-rank thread caps, the final per-read gather — is executed here with all
ranks on device 0 and `gloo` standing in for RCCL (one device cannot host several RCCL ranks).  N = 4, not the driver's 8: with
the pytest process that is five processes holding the one device at once, which a shared test host allows, where nine are too
many; the 8-way LPT split of the whole batch is checked on the CPU (tests/test_synth_and_sharding.py).  Infrastructure, not parity:
tests/conftest.py runs this file after every oracle comparison.  The reference has nothing to rehearse against: f5c is one device
per process (docs/f5c.1:271, --cuda-dev-id)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKS = 4


def _line(stdout):
    return json.loads([ln for ln in stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_zz_four_ranks_on_one_device(tmp_path):
    import bench
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("ABEA_HOST_THREADS", None)                           # the per-rank cap is bench.py's to set
    common = ["--config", "r9_100k_mixed", "--reads", "8000", "--steps", "2", "--warmup", "1", "--one-device", "--arena-gib", "6",
              "--no-cpu-baseline", "--no-small-batch", "--no-process-chain", "--device-steps", "1"]
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + common, capture_output=True, text=True,
                         env=env, timeout=900)
    assert one.returncode == 0, one.stderr[-3000:]
    ref = _line(one.stdout)
    port = 29700 + os.getpid() % 200
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(RANKS), "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(RANKS), "--backend", "gloo"] + common,
                       capture_output=True, text=True, env=env, timeout=1500)
    assert r.returncode == 0, r.stderr[-4000:]
    j = _line(r.stdout)
    # ONE batch, strong-scaled: every event and read of the single-rank run is accounted for, in RANKS LPT shards
    assert j["n_gpus"] == RANKS and j["scaling"] == "strong" and j["value"] > 0 and j["bound"] in bench.BOUND_VALUES
    assert j["config"]["reads"] == 8000 == ref["config"]["reads"] and j["config"]["events"] == ref["config"]["events"]
    assert len(j["per_rank"]) == RANKS and sorted(p["rank"] for p in j["per_rank"]) == list(range(RANKS))
    assert sum(p["events"] for p in j["per_rank"]) == ref["config"]["events"]
    ev = [p["events"] for p in j["per_rank"]]
    assert max(ev) < 1.10 * (sum(ev) / RANKS)                     # LPT on 3 x read length: within 10 % at 2000 reads per rank
    # every read's n_pairs equals the single-rank run's, through the final gather
    assert j["n_pairs"]["shards_partition_the_batch"] is True and j["n_pairs"]["reads"] == 8000
    assert j["n_pairs"]["sha256"] == ref["n_pairs"]["sha256"] and j["n_pairs"]["sum"] == ref["n_pairs"]["sum"]
    assert abs(j["qc_pass_frac"] - ref["qc_pass_frac"]) < 1e-9
    # the host side of the ranks stays inside the CPU quota: busy threads (caller + workers) x ranks <= usable CPUs
    hb = j["host_thread_budget"]
    assert hb["ranks"] == RANKS and len(hb["threads_per_rank_incl_caller"]) == RANKS and min(hb["threads_per_rank_incl_caller"]) >= 1
    if hb["quota_cpus"] >= 16:
        assert hb["within_quota"] and hb["total"] <= hb["quota_cpus"], hb
    assert "nr_throttled" in j["cgroup_cpu"]["in_timed_region"] and "throttled_usec" in j["cgroup_cpu"]["in_timed_region"]
    assert j["collective"]["world"] == RANKS and j["collective"]["backend"] == "gloo"
    # whole-job rates of the legs without host traffic are present for the scaling table of DESIGN §6
    assert j["device_resident"]["mevents_per_s"] > 0 and j["kernel_only"]["mevents_per_s"] > 0
    assert all(0 < x <= 1 for x in _fracs(j)), [x for x in _fracs(j) if not 0 < x <= 1]


def _fracs(obj, key="frac"):
    """every `frac` anywhere in the line (round-5 verdict item 4: none may exceed 1)"""
    out = []
    if isinstance(obj, dict):
        for k_, v in obj.items():
            if k_ == key and isinstance(v, (int, float)):
                out.append(v)
            else:
                out += _fracs(v, key)
    elif isinstance(obj, list):
        for v in obj:
            out += _fracs(v, key)
    return out
