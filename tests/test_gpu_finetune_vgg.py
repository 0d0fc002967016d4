"""GPU: finetune_y4m with the perceptual term on the shared 3-frame 32x32 clip of
tests/finetune_clip.py -- augment off, batch 1, keyed synthetic net weights, keyed synthetic VGG
weights at reduced widths -- against the CPU loop, and the command line.

Bound of the step-0 agreement: 4 x 1.2e-4 relative, the floor of tests/test_gpu_perceptual.py's bound
(12 convs at the 1e-5 of tests/test_gpu_train.py); the fp32 CPU run's own error is below that floor
there, so the larger-of is the floor.

The 8-step CPU loop's total loss falls monotonically with these keyed weights (the values are in
DESIGN.md section 8c), so descent is asserted on both devices."""
import io
import os
import subprocess
import sys

import pytest
import torch

from rrin_amd import Net
from rrin_amd import finetune as ft
from rrin_amd import perceptual as pc
from tests.finetune_clip import DESCENT, clip_bytes, keyed_net

pytestmark = pytest.mark.gpu

SMALL = (4, 4, "M", 8, 8, "M", 8, 8, 8, 8, "M", 16, 16, 16, 16)
BOUND = 4 * 12 * 1e-5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def quiet(*a):
    pass


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("ftvgg")
    raw = clip_bytes(32, 32, 3)
    vgg = pc.VggFeatures.synthetic(SMALL)
    out = {"raw": raw, "dir": d}
    out["plain"] = ft.finetune_y4m(keyed_net(gpu), io.BytesIO(raw), **DESCENT, save=str(d / "plain.pth"), log=quiet)
    out["none"] = ft.finetune_y4m(keyed_net(gpu), io.BytesIO(raw), **DESCENT, save=str(d / "none.pth"), log=quiet,
                                  vgg=None)
    logs = []
    out["vgg"] = ft.finetune_y4m(keyed_net(gpu), io.BytesIO(raw), **DESCENT, save=str(d / "vgg.pth"), log=logs.append,
                                 vgg=vgg, log_every=4)
    out["logs"] = logs
    out["cpu"] = ft.finetune_y4m(keyed_net(), io.BytesIO(raw), **DESCENT, log=quiet, vgg=vgg)
    return out


def state(path):
    return torch.load(path, map_location="cpu", weights_only=True)["model"]


def test_without_vgg_nothing_changes(runs):
    a, b = state(runs["dir"] / "plain.pth"), state(runs["dir"] / "none.pth")
    assert all(a[k].numpy().tobytes() == b[k].numpy().tobytes() for k in a) and len(a) == 162
    assert runs["plain"]["losses"] == runs["none"]["losses"]
    for res in (runs["plain"], runs["none"]):
        assert res["vgg"] is None and res["w_vgg"] is None and res["perceptual"] == []
        assert all("perceptual" not in row for row in res["logged"])


def test_step0_total_is_the_cpu_loops(runs):
    g, c = runs["vgg"], runs["cpu"]
    plain = runs["plain"]["losses"][0]   # step 0 runs on the same weights: the frame loss alone
    print("GPU losses", g["losses"], "perceptual", g["perceptual"])
    print("CPU losses", c["losses"], "perceptual", c["perceptual"])
    assert abs(g["losses"][0] - c["losses"][0]) <= BOUND * c["losses"][0]
    assert abs(g["perceptual"][0] - c["perceptual"][0]) <= BOUND * c["perceptual"][0]
    # the total is the reference's sum: frame_loss + w_vgg * perceptual
    assert abs(g["losses"][0] - (plain + 0.1 * g["perceptual"][0])) <= 1e-12
    assert g["perceptual"][0] > 0


def test_descent_on_both_devices(runs):
    for res in (runs["cpu"], runs["vgg"]):
        assert len(res["losses"]) == 8 and len(res["perceptual"]) == 8
        assert all(b < a for a, b in zip(res["losses"], res["losses"][1:])), res["losses"]


def test_report_fields(runs):
    res = runs["vgg"]
    assert res["vgg"] == "synthetic" and res["w_vgg"] == 0.1
    assert [row["step"] for row in res["logged"]] == [4, 8]
    assert [row["perceptual"] for row in res["logged"]] == [res["perceptual"][3], res["perceptual"][7]]
    assert sum("vgg" in line for line in runs["logs"]) == 2


def test_checkpoint_loads_and_differs(runs, gpu):
    a, b = state(runs["dir"] / "vgg.pth"), state(runs["dir"] / "plain.pth")
    fresh = Net()
    fresh.load_state_dict(a, strict=True)
    assert any(a[k].numpy().tobytes() != b[k].numpy().tobytes() for k in a)
    assert all(bool(torch.isfinite(v).all()) for v in a.values())


def cli_args(d, vgg_path, clip="clip.y4m"):
    return ["--model_name", "M", "finetune", "--y4m_in", str(d / clip), "--steps", "1", "--batch", "1", "--crop", "32",
            "--no_augment", "--val_fraction", "0", "--vgg_weights", str(vgg_path), "--vgg_cfg",
            ",".join(str(v) for v in SMALL), "--report", str(d / "report.json")]


def test_cli_runs_one_step(runs, gpu, tmp_path, monkeypatch, capsys):
    import json

    from rrin_amd.__main__ import main
    (tmp_path / "models").mkdir()
    torch.save({"model": keyed_net().state_dict(), "epoch": 3}, tmp_path / "models" / "M0003.pth")
    (tmp_path / "clip.y4m").write_bytes(runs["raw"])
    torch.save(pc.VggFeatures.synthetic(SMALL).state_dict(), tmp_path / "vgg-small.pth")
    monkeypatch.chdir(tmp_path)
    main(cli_args(tmp_path, tmp_path / "vgg-small.pth"))
    capsys.readouterr()
    rep = json.load(open(tmp_path / "report.json"))
    assert rep["vgg"] == "vgg-small.pth" and rep["w_vgg"] == 0.1 and len(rep["perceptual"]) == 1
    assert abs(rep["losses"][0] - runs["vgg"]["losses"][0]) <= 1e-12   # the same step 0 as the call
    assert os.path.exists(tmp_path / "models" / "M0004.pth")
    # the real widths are what a file is checked against by default: this one mismatches, before the clip
    args = cli_args(tmp_path, tmp_path / "vgg-small.pth", clip="no-such-clip.y4m")
    args = args[:args.index("--vgg_cfg")] + args[args.index("--vgg_cfg") + 2:]
    with pytest.raises(ValueError, match="features.0.weight"):
        main(args)


def test_cli_missing_file_exits_nonzero_before_the_clip(tmp_path):
    """Neither the weights file nor the clip exists: the error is about the weights file."""
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "rrin_amd"] + cli_args(tmp_path, tmp_path / "absent.pth", "no-such-clip.y4m"),
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0
    assert "absent.pth" in p.stderr and "no-such-clip" not in p.stderr
