"""The colour table (stats.run_colour_statistics = SuperresolutionNetwork/mainPSNR4_ColoredNets.py) on the CPU against rows the
reference's own modules produced (tests/golden/make_colour_stats_fixtures.py -> tests/golden/colour_stats_reference.npz): the bilinear
baseline, an unshaded network shaded afterwards and a 56-channel colour network on one PSNR-color / SSIM-color table."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from colour_common import OPT, fill_state_dict
from isosurfacesuperresolution_amd import models, stats

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "colour_stats_reference.npz"))


def generator():
    spec = importlib.util.spec_from_file_location("make_colour_stats_fixtures", os.path.join(HERE, "golden", "make_colour_stats_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                       # (defines functions only; nothing of the reference is imported until main())
    return mod


def write_clips(folder):
    gen = generator()
    clips = gen.colour_stats_clips()
    assert abs(gen.checksum(clips) - float(G["checksum"])) < 1e-6, "other random stream"
    os.makedirs(folder, exist_ok=True)
    for c, (low, high, flow) in enumerate(clips):
        for name, arr in (("low", low), ("high", high), ("flow", flow)):
            np.save(os.path.join(folder, "%s_%05d.npy" % (name, c)), arr)
    return gen


def specs(gen):
    unshaded = fill_state_dict(models.createNetwork('EnhanceNet', 4, 101, [0, 1, 2, 3, 4], 6, OPT).eval(), gen.SEED_UNSHADED)
    colour = fill_state_dict(models.createNetwork('EnhanceNet', 4, 56, [0, 1, 2], 3, OPT).eval(), gen.SEED_COLOUR)
    return [{"name": "bilinear", "path": None}, {"name": "unshaded", "model": unshaded}, {"name": "colour", "model": colour}]


def test_colour_table_reproduces_the_reference_rows(tmp_path):
    folder, out = str(tmp_path / "clips"), str(tmp_path / "results")
    gen = write_clips(folder)
    assert list(G["models"]) == ["bilinear", "unshaded", "colour"]
    res = stats.run_colour_statistics([("Blob", [folder])], specs(gen), out, device="cpu", metric_dtype=torch.float32, log=lambda *a: None)
    for name in G["models"]:
        lines = open(os.path.join(out, "Stats_Blob_%s.txt" % name)).read().splitlines()
        assert lines[0] == "PSNR-color\tSSIM-color" and len(lines) == 1 + gen.CLIPS                   # mainPSNR4_ColoredNets.py:235, one row per clip
        rows = np.array([[float(v) for v in l.split("\t")] for l in lines[1:]])
        ref = G["rows_" + name]
        print(name, "PSNR", np.abs(rows[:, 0] - ref[:, 0]).max(), "dB; MS-SSIM", np.abs(rows[:, 1] - ref[:, 1]).max())
        assert rows.shape == ref.shape == (gen.CLIPS, 2)
        assert np.abs(rows[:, 0] - ref[:, 0]).max() <= 1e-3, (name, rows, ref)                        # the tolerances of test_stats_cpu.py:29-32
        assert np.abs(rows[:, 1] - ref[:, 1]).max() <= 1e-5, (name, rows, ref)
        cols = res["Blob"][name]
        assert cols["PSNR-color"][2] == gen.CLIPS
        assert abs(cols["PSNR-color"][0] - ref[:, 0].mean()) <= 1e-3 and abs(cols["SSIM-color"][0] - ref[:, 1].mean()) <= 1e-5
    summary = open(os.path.join(out, "Summary_Blob.txt")).read().splitlines()
    assert summary[0].split("\t") == ["model", "clips", "PSNR-color-mean", "PSNR-color-var", "SSIM-color-mean", "SSIM-color-var"]
    assert [l.split("\t")[0] for l in summary[1:]] == ["bilinear", "unshaded", "colour"] and summary[1].split("\t")[1] == str(gen.CLIPS)
    assert not os.path.exists(os.path.join(out, "Histogram_Blob_colour.txt"))                          # the script writes none


def test_colour_table_refuses_a_colour_network_without_the_eight_own_channels(tmp_path):
    net = fill_state_dict(models.createNetwork('EnhanceNet', 4, 52, [0, 1, 2], 3, OPT).eval(), 3)
    with pytest.raises(ValueError):
        stats.run_colour_statistics([("Blob", [str(tmp_path)])], [{"name": "c4", "model": net}], str(tmp_path / "out"), device="cpu",
                                    log=lambda *a: None)


def test_hip_metrics_are_refused_without_a_device_or_in_fp32():
    with pytest.raises(ValueError):
        stats.Statistics("cpu", metrics="hip")
    with pytest.raises(ValueError):
        stats.Statistics("cuda", metrics="hip", metric_dtype=torch.float32)
    with pytest.raises(ValueError):
        stats.Statistics("cpu", metrics="fast")
    assert stats.resolve_metrics("auto", "cpu", torch.float64) == "torch" and stats.resolve_metrics("auto", "cuda", torch.float32) == "torch"
