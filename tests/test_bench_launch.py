"""bench.py --gpus N: the self-launch of one rank per GPU (corda_amd/launch.py) and the N > 1 timing /
all-gather machinery, on CPU (gloo).  VERDICT r4 "next round" item 1: `--gpus N` must run N ranks or fail
non-zero, and never print a line whose n_gpus differs from N."""
import json
import os
import subprocess
import sys
import time

import pytest

from corda_amd import launch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    e.update({k: str(v) for k, v in kw.items()})
    return e


def _run(args, env=None, timeout=240):
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout,
                          env=env or _env(), cwd=REPO)


def _line(out: str) -> dict:
    lines = [x for x in out.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.parametrize("world", [2, 3, 8])
def test_self_launch_gathers_over_ranks(world):
    """--gpus N without a launcher starts N ranks (RANK / LOCAL_RANK / WORLD_SIZE set by the parent), every
    timed step all-gathers the ranks' bitmaps, and rank 0's single line reports n_gpus = N."""
    r = _run(["--gpus", str(world), "--plumbing", "--steps", "3", "--warmup", "1", "--n", "6400"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = _line(r.stdout)
    assert d["n_gpus"] == world and d["value"] is None and "no verification" in d["metric"].lower()
    assert d["gathered_words"] == world * 100 and d["gathered_all_ones"]
    assert d["rank_env"]["WORLD_SIZE"] == str(world) and d["rank_env"]["RANK"] == "0"
    assert d["rank_env"]["MASTER_ADDR"] == "127.0.0.1"


def test_gpus_more_than_visible_fails_nonzero():
    """--gpus 2 with fewer than two visible GPUs (this container has none, the GPU box one) exits 2 and names
    the count instead of printing a one-GPU line."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two or more GPUs visible")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], timeout=120)
    assert r.returncode == 2, (r.stdout, r.stderr[-2000:])
    assert "GPU(s) are visible" in r.stderr or "cannot count the GPUs" in r.stderr
    assert not [x for x in r.stdout.splitlines() if x.startswith("{")]


def test_world_size_mismatch_refused():
    """A launcher environment whose WORLD_SIZE differs from --gpus is refused (exit 2), before any GPU call."""
    r = _run(["--gpus", "2", "--plumbing", "--steps", "1"], env=_env(WORLD_SIZE=1, RANK=0, LOCAL_RANK=0))
    assert r.returncode == 2 and "WORLD_SIZE is 1" in r.stderr


def test_launcher_propagates_failure_and_stops_the_rest():
    """One failing rank: spawn returns its status and stops the ranks still running (here one that would
    sleep for a minute) instead of waiting for them."""
    code = ("import os, sys, time\n"
            "r = int(os.environ['RANK'])\n"
            "assert os.environ['WORLD_SIZE'] == '2' and os.environ['LOCAL_RANK'] == str(r)\n"
            "time.sleep(60) if r == 0 else sys.exit(5)\n")
    t = time.monotonic()
    rc = launch.spawn(2, [sys.executable, "-c", code], require_gpus=False)
    assert rc == 5 and time.monotonic() - t < 40


def test_launcher_all_ranks_ok():
    code = "import os, sys; sys.exit(0 if os.environ['MASTER_ADDR'] == '127.0.0.1' else 1)"
    assert launch.spawn(3, [sys.executable, "-c", code], require_gpus=False) == 0


def test_plumbing_noop_verify_fails_the_check():
    """the bitmaps are zeroed after warm-up, so a timed "verify" that writes nothing fails
    the all-ones check (non-zero exit, no line) instead of passing on the warm-up's words."""
    r = _run(["--gpus", "2", "--plumbing", "--plumbing-noop", "--steps", "2", "--warmup", "1", "--n", "640"])
    assert r.returncode != 0, r.stdout
    assert "not written by the timed steps" in r.stderr
    assert not [x for x in r.stdout.splitlines() if x.startswith("{")]


def test_visible_gpus_never_calls_hip(monkeypatch):
    """with no KFD topology and amdsmi failing, the launcher refuses (exit 2) and never
    reaches HIP's device count (torch._C._cuda_getDeviceCount / torch.cuda.device_count), because it forks the
    rank processes afterwards."""
    import torch

    def boom(*a, **k):
        raise AssertionError("HIP device count called by the launcher")

    monkeypatch.setattr(torch._C, "_cuda_getDeviceCount", boom, raising=False)
    monkeypatch.setattr(torch.cuda, "device_count", boom)
    monkeypatch.setattr(launch, "KFD_NODES", "/nonexistent/kfd/topology/nodes")

    class _FailingSmi:
        def amdsmi_init(self):
            raise RuntimeError("amdsmi: no driver")

    monkeypatch.setitem(sys.modules, "amdsmi", _FailingSmi())
    assert launch.visible_gpus() == -1
    assert launch.spawn(2, [sys.executable, "-c", "pass"], require_gpus=True) == 2


def test_dump_outputs_float32_bounded_and_repeatable(tmp_path):
    """--dump-outputs: float32 files; an array past its share of the byte budget is cut to a sample of rows that is
    the same in every run and keeps the rows' order; a small array is written whole."""
    import numpy as np
    sys.path.insert(0, REPO)
    import bench

    rows = 3 * bench.DUMP_BYTES // (2 * 4 * 32)            # 3x its half of the budget at 32 values per row
    big = np.zeros((rows, 32), np.uint8)
    big[:, :4] = np.arange(rows, dtype="<u4").view(np.uint8).reshape(rows, 4)
    big[:, 4:] = (np.arange(rows)[:, None] * 7 + np.arange(28)[None, :]) % 256
    small = np.arange(1000) % 2 == 0
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = (np.load(tmp_path / d / "big.npy") for d in ("a", "b"))
    assert a.dtype == np.float32 and np.array_equal(a, b)
    assert a.shape == (bench.DUMP_BYTES // 2 // (4 * 32), 32)
    # every sampled row is a row of the input (its first three bytes spell its index), in the input's order
    idx = (a[:, 0] + 256 * a[:, 1] + 65536 * a[:, 2]).astype(np.int64)
    assert (np.diff(idx) > 0).all() and idx[-1] < rows and np.array_equal(a, big[idx].astype(np.float32))
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.astype(np.float32))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64_000_000


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_dumps_its_verdicts(tmp_path):
    """A plain run times its steps and prints the headline fields alone (the other legs belong to --full);
    --dump-outputs writes one float32 verdict per signature of the last timed step, all 1 for the honest batch."""
    import numpy as np
    n = 6400 + 37
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--n", str(n), "--dump-outputs", str(tmp_path / "out")])
    assert r.returncode == 0, r.stderr[-2000:]
    d = _line(r.stdout)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["unit"] == "verifies/s"
    assert d["ms_per_step"] > 0 and abs(d["value"] - n / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["higher_is_better"] is True and d["config"]["sigs_per_gpu"] == n
    assert not {"roofline", "cpu_baseline", "host_api", "c3", "c5_shard", "keyed", "notary", "detail_file"} & set(d)
    v = np.load(tmp_path / "out" / "verdicts.npy")
    assert v.dtype == np.float32 and v.shape == (n,) and (v == 1).all()
    assert os.listdir(tmp_path / "out") == ["verdicts.npy"]


def _fake_node(root, idx, simd, minor):
    d = root / str(idx)
    d.mkdir(parents=True)
    (d / "properties").write_text(f"cpu_cores_count 0\nsimd_count {simd}\ndrm_render_minor {minor}\n")


def test_kfd_topology_count(tmp_path, monkeypatch):
    """The sysfs count: GPU nodes (simd_count > 0) whose render node this process can open; CPU nodes and GPUs
    of other containers (render node absent) do not count; the visibility variables restrict the result."""
    nodes, dri = tmp_path / "nodes", tmp_path / "dri"
    dri.mkdir()
    _fake_node(nodes, 0, 0, -1)                          # the CPU node
    for i, minor in enumerate((128, 129, 130, 131)):
        _fake_node(nodes, i + 1, 1024, minor)
    for minor in (128, 130, 131):                        # renderD129 belongs to another container
        (dri / f"renderD{minor}").write_text("")
    assert launch._kfd_gpu_count(str(nodes), str(dri)) == 3
    assert launch._kfd_gpu_count(str(tmp_path / "none"), str(dri)) is None
    for v in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(v, raising=False)
    assert launch._apply_visibility(3) == 3
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,1")
    assert launch._apply_visibility(3) == 2
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0")
    assert launch._apply_visibility(3) == 1
