"""First contact with a multi-GPU box, rehearsed on the one GPU there is: `bench.py --gpus 4 --dry-ranks`
starts FOUR rank processes through torch.distributed.run exactly as the driver's command line does, every rank on GPU 0,
the collectives over gloo (RCCL refuses several ranks on one device).  Everything except RCCL-over-xGMI executes: the
rendezvous, four concurrent part-stream probes, four envs of 8 192 books (the C4 shard size) with their book_offset,
bk_warm, the region / barrier logic, the per-launch stats all-gather and the books_total / ranks_seen consistency checks
of the bench line.  Four ranks, not the eight of an 8-GPU node: a shared GPU takes at most six processes at once.

The children are started BEFORE this pytest process touches the GPU (the file sorts ahead of test_gpu_parity.py)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_four_ranks_dry_run_on_one_gpu():
    env = dict(os.environ, BOURSE_AMD_VERBOSE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-ranks", "--books", "32768",
                        "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--repeats", "1"],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["dry_ranks"] is True and out["n_gpus"] == 4 and out["scaling"] == "strong"
    cfg = out["config"]
    assert cfg["books_total"] == 32768 and cfg["books_per_gpu"] == 8192 and cfg["ranks"] == 4
    assert cfg["stats_allgather"]["ranks_seen"] == 4 and cfg["stats_allgather"]["n_books"] == 32768
    assert cfg["stats_allgather"]["sum_trades"] > 0
    assert cfg["pipeline"].startswith("wave_split")  # the auto rule at the C4 shard size
    assert [d["first_book"] for d in cfg["ranks_detail"]] == [0, 8192, 16384, 24576]
    rr = out["rank_region_ms"]
    assert len(rr["all"]) == 4 and 0 < rr["min"] <= rr["median"] <= rr["max"]
    assert out["value"] > 0 and out["steps"] == 20
    # every rank probed its part streams (four probes at the same time on one device)
    assert r.stderr.count("candidate streams on hardware queues of their own") + r.stderr.count("part streams taken unprobed") >= 4, r.stderr[-3000:]
