"""bench.py pieces that do not need a GPU: the algorithmic work the roofline is priced on, the loud failure without a device, the
--full / --dump-outputs options; and (marked gpu) what a plain run prints and dumps."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("frcnn_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_algorithmic_work_matches_design():
    b = _bench()
    from chainer_faster_rcnn_amd.models.vgg16 import LAYERS
    flops, (fh, fw) = b.conv_flops(LAYERS, b.IM_H, b.IM_W)
    assert (b.IM_H, b.IM_W) == (600, 1000) and (fh, fw) == (38, 63) and len(flops) == 14
    assert abs(sum(flops.values()) / 1e9 - 379.03) < 0.01                        # 13 VGG convs + rpn_conv_3x3
    nbytes = b.conv_algorithmic_bytes(LAYERS, b.IM_H, b.IM_W)
    assert set(nbytes) == set(flops) and abs(sum(nbytes.values()) / 14e6 - 67.5) < 0.1
    assert b.PEAK_F32_MFMA_TFLOPS == 157.3 and b.PEAK_HBM_GBPS == 8000.0


def test_pmc_traffic_comes_from_the_committed_profile():
    b = _bench()
    traffic, src = b.pmc_traffic("f32")
    summary = json.load(open(os.path.join(ROOT, "profiles", "r06_hbm_traffic_pmc.json")))["_summary"]           # the newest committed pass wins
    assert traffic == summary["conv_mfma_f32_kernel"]["hbm_bytes_per_launch"] and "profiles/r06_hbm_traffic_pmc.json" in src
    # the guide's gfx950 correction (FETCH_SIZE halves 16-byte-per-lane reads) is applied: corrected = 2 * fetch + write
    c = summary["conv_mfma_f32_kernel"]
    assert abs(c["hbm_bytes_per_launch"] - (2 * c["fetch_bytes_per_launch_raw"] + c["write_bytes_per_launch"])) < 1.0
    traffic16, src16 = b.pmc_traffic("bf16")
    s16 = json.load(open(os.path.join(ROOT, "profiles", "r06_hbm_traffic_pmc_bf16.json")))["_summary"]["conv_bf16_kernel"]
    assert traffic16 == s16["hbm_bytes_per_launch"] and "bf16" in src16 and "BEFORE the strip-form" not in src16        # this pass measured the shipped picks


def test_split_product_variant_is_reported_next_to_the_contract_line_not_instead_of_it():
    """`value` of the default line is the native fp32 MFMA measurement; the bf16x6 split-product variant (same fp32 network) is a
    second object of the same line, priced on the bf16 MFMA flops it actually executes."""
    b = _bench()
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'res["f32_split_products"] = split_variant(' in src and "--no-split-variant" in src
    assert 'ap.add_argument("--dtype", choices=["f32", "f32s", "bf16", "f16"], default="f32"' in src          # the contract line stays on f32
    traffic, tsrc = b.pmc_traffic("f32s")
    s3 = json.load(open(os.path.join(ROOT, "profiles", "r02_hbm_traffic_pmc_f32s.json")))["_summary"]["conv_f32s_kernel"]
    assert traffic == s3["hbm_bytes_per_launch"] and "f32s" in tsrc
    line = json.load(open(os.path.join(ROOT, "profiles", "r02_bench.json")))
    assert line["dtype"] == "f32" and line["parity"]["ok"] and line["f32_split_products"]["parity"]["ok"]
    assert line["f32_split_products"]["value"] > line["value"]


def test_default_timed_region_is_long_enough_to_be_seen():
    b = _bench()
    assert b.DEFAULT_STEPS >= 200                    # ~1 s at 3.8 ms / step (gpu_busy saw nothing in a 0.08 s window)


def test_bench_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and not r.stdout.strip().startswith("{")            # no number is better than a CPU-fallback number


def test_gpus8_launch_and_rank_placement_dry():
    """`bench.py --gpus 8` without a launcher becomes the driver's own command (one rank per GPU of one node, 127.0.0.1 rendezvous), and each of its
    eight ranks maps LOCAL_RANK -> its own device over RCCL (the first 8-GPU run must not be the first execution of this logic)."""
    b = _bench()
    cmd = b.launch_command(8, 29517, ["--gpus", "8", "--steps", "20", "--warmup", "5"])
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and cmd[4:6] == ["--nproc-per-node", "8"]
    assert cmd[6:10] == ["--master-addr", "127.0.0.1", "--master-port", "29517"]
    assert cmd[10] == os.path.join(ROOT, "bench.py") and cmd[11:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]
    seen = set()
    for r in range(8):
        env = {"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": "8", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29517"}
        rank, local_rank, world, device, backend, note = b.rank_placement(env, 8, 8)
        assert (rank, local_rank, world, device, backend, note) == (r, r, 8, r, "nccl", None)
        seen.add(device)
    assert seen == set(range(8))
    # 8 ranks on a 1-GPU box: gloo, every rank on device 0, and the line says it is not a scaling number
    rank, _, world, device, backend, note = b.rank_placement({"RANK": "5", "LOCAL_RANK": "5", "WORLD_SIZE": "8"}, 8, 1)
    assert (rank, world, device, backend) == (5, 8, 0, "gloo") and "not a scaling number" in note
    # a launcher / flag mismatch and a rank without a device fail loudly instead of double-booking a GPU
    with pytest.raises(SystemExit):
        b.rank_placement({"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "4"}, 8, 8)
    with pytest.raises(SystemExit):
        b.rank_placement({"RANK": "9", "LOCAL_RANK": "9", "WORLD_SIZE": "8"}, 8, 8)
    # no launcher, one GPU: rank 0 of a world of one
    assert b.rank_placement({}, 1, 1)[:4] == (0, 0, 1, 0)


def test_every_baseline_config_line_carries_roofline_and_cpu_baseline():
    """VERDICT r05 missing #4: the RPN training line (BASELINE configs[4]), the stage-2 line and the ResNet-101 line (configs[3]) state their roofline
    fraction and a CPU baseline timed in the same run, like the contract line -- checked on the committed round-6 records and on the code that makes them."""
    b = _bench()
    from chainer_faster_rcnn_amd.models.vgg16 import LAYERS
    f = b.train_flops(LAYERS, 600, 1000)
    assert abs(sum(f.values()) / 1e12 - 1.135) < 0.001 and abs(f["input_gradients"] - (f["forward"] - 2.0 * 600 * 1000 * 64 * 3 * 9)) < 1.0   # conv1_1 has no input gradient
    f2 = b.train_flops(LAYERS, 600, 1000, stage2=True, n_rois=300, bwd_rows=128)
    assert abs(f2["forward"] / 1e9 - (379.03 + 2e-9 * 300 * (25088 * 4096 + 4096 * 4096))) < 0.01
    for name, key in (("r06_bench_train.json", "ms_per_step"), ("r06_bench_train_rcnn_device.json", "ms_per_step"), ("r06_bench_resnet101.json", "ms_per_image")):
        line = json.loads(open(os.path.join(ROOT, "profiles", name)).read().strip().splitlines()[-1])
        r, c = line["roofline"], line["cpu_baseline"]
        assert r["bound"] == "mfma" and r["peak"] == 157.3 and 0.2 < r["frac"] < 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9, name
        assert c["unit"] == "img/s" and c["value"] > 0 and c["cores"] >= 1 and c["kind"] in ("reference-native", "port") and c[key] > 100 and "sample" in c, name


def test_full_and_dump_outputs_options():
    """`--full` (every secondary measurement) and `--dump-outputs DIR` are options of the benchmark; --help works without a GPU."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    import torch
    b = _bench()
    out = {"cls_prob": np.ones((300, 21), np.float32), "rois": np.zeros((300, 4), np.float32), "n_out": np.array([7], np.int32),
           "probs": np.ones(300, np.float32)}
    res = b.inference_outputs(type("R", (), {"mem": type("M", (), {"to_numpy": staticmethod(np.asarray)})()})(),
                              dict(out, pred_boxes=np.ones((300, 84), np.float32)))
    assert [res[k].shape[0] for k in ("cls_prob", "pred_boxes", "rois", "probs")] == [7] * 4 and res["n_out"].tolist() == [7.0]
    names = b.dump_outputs(str(tmp_path / "d"), res)
    assert names == ["cls_prob", "n_out", "pred_boxes", "probs", "rois"]
    for n in names:
        a = np.load(str(tmp_path / "d" / (n + ".npy")))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, res[n])
    with pytest.raises(ValueError):
        b.dump_outputs(str(tmp_path / "big"), {"w": np.zeros(b.DUMP_LIMIT_BYTES // 4 + 1, np.float32)})
    # a large flat buffer: the same seeded sample every time, at most DUMP_SAMPLE elements
    flat = torch.arange(3 * b.DUMP_SAMPLE, dtype=torch.float32)
    s1, s2 = b.flat_sample(torch, flat), b.flat_sample(torch, flat)
    assert np.array_equal(s1, s2) and 0.5 * b.DUMP_SAMPLE < len(s1) <= b.DUMP_SAMPLE and np.all(np.diff(s1) > 0)
    assert np.array_equal(b.flat_sample(torch, flat[:100]), np.arange(100, dtype=np.float32))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_forward(tmp_path):
    """A plain run: the line carries the contract fields and `steps` = --steps, none of the --full blocks; --dump-outputs holds the
    forward's valid rows, equal to an eager forward of the same seeded image and weights."""
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 * line["value"] and line["unit"] == "img/s"
    assert not {"roofline", "cpu_baseline", "parity", "bf16_config3", "f32_split_products", "with_feed", "stages_ms"} & set(line)
    import chainer_faster_rcnn_amd as pkg
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.models import FasterRCNN
    b = _bench()
    rt = pkg.runtime.default_runtime()
    model = FasterRCNN(runtime=rt)
    model.load_params(synthetic.params(seed=1))
    want = b.inference_outputs(rt, model.forward_device(rt.mem.from_numpy(synthetic.image(seed=0, h=b.IM_H, w=b.IM_W)), b.IM_H, b.IM_W))
    assert sorted(p.name for p in d.iterdir()) == sorted(k + ".npy" for k in want)
    for k, v in want.items():
        got = np.load(str(d / (k + ".npy")))
        assert got.dtype in (np.float32, np.float64) and got.shape == v.shape, k
        assert np.allclose(got, v, rtol=1e-5, atol=1e-5), k
