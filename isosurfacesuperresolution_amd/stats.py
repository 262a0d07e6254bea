"""Statistics harness: run super-resolution models over a set of clips and tabulate PSNR / MS-SSIM / down-sampling consistency per
channel group -- what ``SuperresolutionNetwork/mainPSNR3_AllStats.py`` does.

Restated pieces (reference file:line):

* baseline "models" nearest / bilinear / bicubic (``SimpleUpsample``, ``:71-97``);
* per clip and model the temporal recurrence of ``:302-346``: frame 0 starts from ``initialImage(.., 'zero')``, frame j > 0 from the
  previous prediction warped with the dataset's flow ``flow[j - 1]`` (``warp_upscale(.., special_mask=True)``), the prediction is
  clamped / normalised (mask to [-1, 1], unit normals, depth and AO to [0, 1]) and fed back;
* ``Statistics`` (``:129-299``): shading with and without ambient occlusion (the set-up of ``:104-116``), a border of 15 low-resolution
  pixels cut off, frames whose ground-truth mask covers less than 5 % skipped, masked PSNR (``utils/psnr.py``) of normal / depth / AO /
  colour, MS-SSIM (``utils/ssim.py``) of the same groups after the prediction was blended with the ground truth outside the mask, the
  L2 distance between the low-resolution input and the down-sampled prediction (normal, colour), L1-error histograms with 200 bins;
* output: one ``Stats_<dataset>_<model>.txt`` per model -- a header and ONE ROW PER CLIP with the 14 tab-separated columns of
  ``:160-163,270-281`` -- and one ``Histogram_<dataset>_<model>.txt`` (``:283-299``).

Metric precision.  The reference evaluates PSNR and MS-SSIM in fp32 on whatever device it runs on.  MS-SSIM forms local variances
as E[x^2] - E[x]^2 under an 11-tap window: on a nearly constant channel (depth, AO) that is a cancellation against C2 = 9e-4, and two
fp32 convolution implementations -- torch's CPU kernel and its device kernel -- disagree by up to 3e-4 in the MS-SSIM of IDENTICAL
images (measured on the bilinear baseline, where no kernel of this package runs).  ``metric_dtype`` (default float64) is the
precision the metrics are evaluated in: in fp64 the table depends on the predictions only, so the HIP run and the CPU run of the
same model agree to 1e-5 (``tests/test_stats_gpu.py``); ``metric_dtype=torch.float32`` is the reference's arithmetic.

Added here: every per-clip quantity also goes into a ``utils.MeanVariance`` accumulator per model (``utils/mv.py``), returned by
``run_statistics`` and written as ``Summary_<dataset>.txt`` (mean and variance over the clips) -- the reference leaves that
aggregation to a spreadsheet.

Metric stage.  ``Statistics(metrics="hip")`` evaluates the five PSNR, the five MS-SSIM columns and the six histograms with the kernels
of ``csrc/sr_metrics.hip`` (``ops.masked_sq_err``, ``ops.msssim_terms``, ``ops.abs_diff_histogram``): fp64 arithmetic on the fp32 frames
where they lie (the cropped views, no fp64 copy of a full-resolution image), sums and histograms kept on the device until a row is
written, one ``.item()`` per frame (the fill check).  It needs a CUDA device and ``metric_dtype=float64``; ``"torch"`` (the default)
is the code above as it always was.

The colour table.  ``run_colour_statistics`` is ``SuperresolutionNetwork/mainPSNR4_ColoredNets.py``: interpolation baselines, unshaded
networks (shaded afterwards) and the colour (RGB) networks on ONE colour PSNR / MS-SSIM table -- INTEGRATION.md section 3 has the
line-by-line table.  ``load_models`` / ``run_statistics`` keep refusing colour models: their columns are those of the G-buffer.

On a CUDA device the networks run on the HIP kernels (``models.EnhanceNet.forward`` -> ``ops.conv3x3`` ...), the warp is the module
path's (bit-identical to the frame pipeline's fused kernel).  This is an OFFLINE renderer in the sense of INTEGRATION.md section 4:
the last frame of every clip is followed by ``ops.guards_flush``.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .inference.loadedmodel import guarded_forward
from .train import clip_recurrence
from .utils import MSSSIM, PSNR, MeanVariance, ScreenSpaceShading, clamp_prediction

UPSCALING = 4
BORDER = 15
MIN_FILLING = 0.05
NUM_BINS = 200
COLUMNS = ("PSNR-normal", "PSNR-depth", "PSNR-ao", "PSNR-color-noAO", "PSNR-color-withAO",
           "SSIM-normal", "SSIM-depth", "SSIM-ao", "SSIM-color-noAO", "SSIM-color-withAO",
           "L2-ds-normal-mean", "L2-ds-normal-max", "L2-ds-color-noAO-mean", "L2-ds-color-noAO-max")


class SimpleUpsample(nn.Module):
    """The interpolation baselines (``mainPSNR3_AllStats.py:71-97``): the five input channels resized, AO = 1."""

    def __init__(self, upscale_factor, upsample):
        super().__init__()
        self.upscale_factor, self.upsample = upscale_factor, upsample
        self.input_channels, self.output_channels = 5, 6

    def forward(self, inputs):
        inputs = inputs[:, 0:self.input_channels]
        size = [inputs.shape[2] * self.upscale_factor, inputs.shape[3] * self.upscale_factor]
        kw = {} if self.upsample == "nearest" else {"align_corners": False}
        resized = F.interpolate(inputs, size=size, mode=self.upsample, **kw)
        ones = torch.ones(resized.shape[0], self.output_channels - self.input_channels, resized.shape[2], resized.shape[3],
                          dtype=resized.dtype, device=resized.device)
        return torch.cat([resized, ones], dim=1), None


def default_shading(device):
    """``mainPSNR3_AllStats.py:104-116``."""
    sh = ScreenSpaceShading(device)
    sh.fov(30)
    sh.ambient_light_color(np.array([0.1, 0.1, 0.1]))
    sh.diffuse_light_color(np.array([1.0, 1.0, 1.0]))
    sh.specular_light_color(np.array([0.0, 0.0, 0.0]))
    sh.specular_exponent(16)
    sh.light_direction(np.array([0.1, 0.1, 1.0]))
    sh.material_color(np.array([1.0, 0.3, 0.0]))
    sh.ambient_occlusion(1.0)
    sh.inverse_ao = False
    return sh


def colour_shading(device):
    """``mainPSNR4_ColoredNets.py:99-109``: the colour table's shading -- white material, no ambient occlusion."""
    sh = ScreenSpaceShading(device)
    sh.fov(30)
    sh.ambient_light_color(np.array([0.1, 0.1, 0.1]))
    sh.diffuse_light_color(np.array([0.9, 0.9, 0.9]))
    sh.specular_light_color(np.array([0.02, 0.02, 0.02]))
    sh.specular_exponent(16)
    sh.light_direction(np.array([0.1, 0.1, 1.0]))
    sh.material_color(np.array([1.0, 1.0, 1.0]))
    sh.ambient_occlusion(0.0)
    sh.inverse_ao = False
    return sh


def check_metrics(metrics, device, metric_dtype):
    """``metrics``: "torch" (the fp64 / fp32 torch operations) or "hip" (the kernels of csrc/sr_metrics.hip: a CUDA device, fp64)."""
    if metrics not in ("torch", "hip"):
        raise ValueError("metrics must be 'torch' or 'hip', not %r" % (metrics,))
    if metrics == "hip" and not (str(device).startswith("cuda") and metric_dtype == torch.float64):
        raise ValueError("metrics='hip' needs a CUDA device and metric_dtype=torch.float64 (device %s, %s)" % (device, metric_dtype))


def resolve_metrics(metrics, device, metric_dtype):
    """"auto": the kernels where they apply (a CUDA device, fp64 metrics -- profiles/stats_metrics.md), the torch operations otherwise."""
    if metrics == "auto":
        return "hip" if str(device).startswith("cuda") and metric_dtype == torch.float64 else "torch"
    return metrics


class Statistics:
    """Accumulators of one model (``mainPSNR3_AllStats.py:129-299``).  ``add_timestep_sample`` per frame, ``write_sample`` per clip."""

    def __init__(self, device, shading=None, upscaling=UPSCALING, border=BORDER, min_filling=MIN_FILLING, ao_strength=1.0,
                 metric_dtype=torch.float64, metrics="torch"):
        check_metrics(metrics, device, metric_dtype)
        self.device = device
        self.metric_dtype = metric_dtype
        self.metrics = metrics
        self.shading = shading if shading is not None else default_shading(device)
        self.upscaling, self.border, self.min_filling, self.ao_strength = upscaling, border, min_filling, ao_strength
        self.ssim = MSSSIM().to(device)
        self.psnr = PSNR().to(device)
        self.histograms = {k: np.zeros(NUM_BINS, dtype=np.float64) for k in ("mask", "normal", "depth", "ao", "color_withAO", "color_noAO")}
        self.histogram_counter = 0
        self.clips = {c: MeanVariance() for c in COLUMNS}          # over the clips written so far
        if metrics == "hip":                                       # sums and histograms stay on the device until a row is written
            self._is_max = torch.tensor([c.endswith("-max") for c in COLUMNS], device=device)
            self._dev_histograms = torch.zeros(len(self.histograms), NUM_BINS, dtype=torch.float64, device=device)
            self._tables = {}                                      # (H, W) -> MS-SSIM windows; the histogram edges
        self.reset()

    def reset(self):
        self.n = 0
        self.sums = dict.fromkeys(COLUMNS, 0.0)
        if self.metrics == "hip":
            self._dev_sums = torch.zeros(len(COLUMNS), dtype=torch.float64, device=self.device)

    @staticmethod
    def write_header(file):
        file.write("\t".join(COLUMNS) + "\n")

    def _downsample(self, t):
        # nn.Upsample(scale_factor=1/UPSCALING, mode='bilinear') of :133-134
        return F.interpolate(t, scale_factor=1.0 / self.upscaling, mode='bilinear', align_corners=False)

    def add_timestep_sample(self, pred_mnda, gt_mnda, input_mnda):
        """pred / gt: [1, 6, H, W] mask, normal, depth, AO at the high resolution; input: [1, 5, h, w] the low-resolution frame."""
        if self.metrics == "hip":
            return self._add_timestep_sample_hip(pred_mnda, gt_mnda, input_mnda)
        sh = self.shading
        sh.ambient_occlusion(self.ao_strength)
        pred_c_ao, gt_c_ao = sh(pred_mnda), sh(gt_mnda)
        sh.ambient_occlusion(0.0)
        pred_c, gt_c, in_c = sh(pred_mnda), sh(gt_mnda), sh(input_mnda)
        sh.ambient_occlusion(self.ao_strength)
        b, b2 = self.border, self.border * self.upscaling
        cut = (lambda t, k: t[:, :, k:-k, k:-k]) if b > 0 else (lambda t, k: t)
        pred_mnda, pred_c_ao, pred_c = cut(pred_mnda, b2), cut(pred_c_ao, b2), cut(pred_c, b2)
        gt_mnda, gt_c_ao, gt_c = cut(gt_mnda, b2), cut(gt_c_ao, b2), cut(gt_c, b2)
        input_mnda, in_c = cut(input_mnda, b), cut(in_c, b)
        md = self.metric_dtype                                      # shading above runs in the tensors' own precision; the METRICS in `md`
        pred_mnda, pred_c_ao, pred_c, gt_mnda, gt_c_ao, gt_c, input_mnda, in_c = (
            t.to(md) for t in (pred_mnda, pred_c_ao, pred_c, gt_mnda, gt_c_ao, gt_c, input_mnda, in_c))
        mask = gt_mnda[:, 0:1] * 0.5 + 0.5
        _, _, H, W = mask.shape
        if torch.sum(mask).item() / (H * W) < self.min_filling:
            return False                                            # too few filled pixels (:208-211)
        self.n += 1
        s = self.sums
        s["PSNR-normal"] += self.psnr(pred_mnda[:, 1:4], gt_mnda[:, 1:4], mask=mask).item()
        s["PSNR-depth"] += self.psnr(pred_mnda[:, 4:5], gt_mnda[:, 4:5], mask=mask).item()
        s["PSNR-ao"] += self.psnr(pred_mnda[:, 5:6], gt_mnda[:, 5:6], mask=mask).item()
        s["PSNR-color-withAO"] += self.psnr(pred_c_ao, gt_c_ao, mask=mask).item()
        s["PSNR-color-noAO"] += self.psnr(pred_c, gt_c, mask=mask).item()
        pred_mnda = gt_mnda + mask * (pred_mnda - gt_mnda)          # SSIM sees the ground truth outside the mask (:223)
        s["SSIM-normal"] += self.ssim(pred_mnda[:, 1:4], gt_mnda[:, 1:4]).item()
        s["SSIM-depth"] += self.ssim(pred_mnda[:, 4:5], gt_mnda[:, 4:5]).item()
        s["SSIM-ao"] += self.ssim(pred_mnda[:, 5:6], gt_mnda[:, 5:6]).item()
        s["SSIM-color-withAO"] += self.ssim(pred_c_ao, gt_c_ao).item()
        s["SSIM-color-noAO"] += self.ssim(pred_c, gt_c).item()
        ds_normal = (input_mnda[:, 1:4] - ScreenSpaceShading.normalize(self._downsample(pred_mnda[:, 1:4]), dim=1)) ** 2
        ds_color = (in_c - self._downsample(pred_c)) ** 2
        s["L2-ds-normal-mean"] += torch.mean(ds_normal).item()
        s["L2-ds-normal-max"] = max(s["L2-ds-normal-max"], torch.max(ds_normal).item())
        s["L2-ds-color-noAO-mean"] += torch.mean(ds_color).item()
        s["L2-ds-color-noAO-max"] = max(s["L2-ds-color-noAO-max"], torch.max(ds_color).item())
        self.histogram_counter += 1
        for key, diff in (("mask", (gt_mnda[0, 0] - pred_mnda[0, 0]).abs()),
                          ("normal", (gt_mnda[0, 1:4] - pred_mnda[0, 1:4]).abs().sum(dim=0) / 6),
                          ("depth", (gt_mnda[0, 4] - pred_mnda[0, 4]).abs()), ("ao", (gt_mnda[0, 5] - pred_mnda[0, 5]).abs()),
                          ("color_withAO", (gt_c_ao[0, 0] - pred_c_ao[0, 0]).abs()), ("color_noAO", (gt_c[0, 0] - pred_c[0, 0]).abs())):
            h, _ = np.histogram(diff.detach().cpu().numpy(), bins=NUM_BINS, range=(0, 1), density=True)
            self.histograms[key] += (h / NUM_BINS - self.histograms[key]) / self.histogram_counter
        return True

    def _metric_tables(self, H, W):
        from . import ops
        if "edges" not in self._tables:
            self._tables["edges"] = ops.histogram_edges(NUM_BINS, self.device)
        if (H, W) not in self._tables:
            self._tables[(H, W)] = ops.msssim_windows(H, W, self.device)
        return self._tables[(H, W)], self._tables["edges"]

    def _add_timestep_sample_hip(self, pred_mnda, gt_mnda, input_mnda):
        """The same frame with the metric kernels: the full-resolution images stay fp32 views, every metric is evaluated in fp64 by
        ``ops.masked_sq_err`` / ``ops.msssim_terms`` / ``ops.abs_diff_histogram`` (the blend of :223 happens on load), nothing but the
        fill check is read back."""
        from . import ops
        sh = self.shading
        sh.ambient_occlusion(self.ao_strength)
        pred_c_ao, gt_c_ao = sh(pred_mnda), sh(gt_mnda)
        sh.ambient_occlusion(0.0)
        pred_c, gt_c, in_c = sh(pred_mnda), sh(gt_mnda), sh(input_mnda)
        sh.ambient_occlusion(self.ao_strength)
        b, b2 = self.border, self.border * self.upscaling
        cut = (lambda t, k: t[:, :, k:-k, k:-k]) if b > 0 else (lambda t, k: t)
        pred, pred_c_ao, pred_c = cut(pred_mnda, b2).float(), cut(pred_c_ao, b2), cut(pred_c, b2)
        gt, gt_c_ao, gt_c = cut(gt_mnda, b2).float(), cut(gt_c_ao, b2), cut(gt_c, b2)
        md = self.metric_dtype
        input_mnda, in_c = cut(input_mnda, b).to(md), cut(in_c, b).to(md)
        mask = gt[0, 0].to(md) * 0.5 + 0.5                          # ONE fp64 plane: PSNR mask, SSIM / histogram blend
        H, W = mask.shape
        if torch.sum(mask).item() / (H * W) < self.min_filling:
            return False
        self.n += 1
        windows, edges = self._metric_tables(H, W)

        def psnr(a, g):
            return ops.psnr_from_sq_err(ops.masked_sq_err(a, g, mask), a.shape[1], H, W, masked=True)

        def ssim(a, g, blend):
            return ops.msssim_terms(a, g, blend=blend, windows=windows)[-1]
        row = [psnr(pred[:, 1:4], gt[:, 1:4]), psnr(pred[:, 4:5], gt[:, 4:5]), psnr(pred[:, 5:6], gt[:, 5:6]),
               psnr(pred_c, gt_c), psnr(pred_c_ao, gt_c_ao),
               ssim(pred[:, 1:4], gt[:, 1:4], mask), ssim(pred[:, 4:5], gt[:, 4:5], mask), ssim(pred[:, 5:6], gt[:, 5:6], mask),
               ssim(pred_c, gt_c, None), ssim(pred_c_ao, gt_c_ao, None)]
        # L2-ds: nn.Upsample(1 / r, 'bilinear') of an image r times as large reads, per low-resolution pixel, the 2 x 2 pixels around its
        # centre with weight 1/2 each way (r even) -- gathered as four low-resolution strided views, blended and averaged in fp64 in the
        # order of the resize kernel
        r = self.upscaling
        if r % 2 == 0:
            o = r // 2 - 1

            def down(value):
                v00, v01, v10, v11 = (value(lambda t: t[..., o + dy::r, o + dx::r].to(md)) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)))
                return 0.5 * (0.5 * v00 + 0.5 * v01) + 0.5 * (0.5 * v10 + 0.5 * v11)
        else:
            def down(value):
                return self._downsample(value(lambda t: t.to(md)))
        down_normal = down(lambda tap: tap(gt[:, 1:4]) + tap(mask) * (tap(pred[:, 1:4]) - tap(gt[:, 1:4])))
        ds_normal = (input_mnda[:, 1:4] - ScreenSpaceShading.normalize(down_normal, dim=1)) ** 2
        ds_color = (in_c - down(lambda tap: tap(pred_c))) ** 2
        row += [torch.mean(ds_normal), torch.max(ds_normal), torch.mean(ds_color), torch.max(ds_color)]
        row = torch.stack(row)
        self._dev_sums = torch.where(self._is_max, torch.maximum(self._dev_sums, row), self._dev_sums + row)
        self.histogram_counter += 1
        counts = torch.stack([ops.abs_diff_histogram(pred[:, 0:1], gt[:, 0:1], NUM_BINS, blend=mask, edges=edges),
                              ops.abs_diff_histogram(pred[:, 1:4], gt[:, 1:4], NUM_BINS, scale=1.0 / 6.0, blend=mask, edges=edges),
                              ops.abs_diff_histogram(pred[:, 4:5], gt[:, 4:5], NUM_BINS, blend=mask, edges=edges),
                              ops.abs_diff_histogram(pred[:, 5:6], gt[:, 5:6], NUM_BINS, blend=mask, edges=edges),
                              ops.abs_diff_histogram(pred_c_ao[:, 0:1], gt_c_ao[:, 0:1], NUM_BINS, edges=edges),
                              ops.abs_diff_histogram(pred_c[:, 0:1], gt_c[:, 0:1], NUM_BINS, edges=edges)])
        masses = counts[:, :NUM_BINS].to(torch.float64) / counts[:, NUM_BINS:].to(torch.float64)
        self._dev_histograms += (masses - self._dev_histograms) / self.histogram_counter
        return True

    def sample_row(self):
        if self.metrics == "hip":
            self.sums = dict(zip(COLUMNS, self._dev_sums.tolist()))
        n = max(1, self.n)
        return [self.sums[c] if c.endswith("-max") else self.sums[c] / n for c in COLUMNS]

    def write_sample(self, file):
        """All frames of a clip were added: one row (``:270-281``), fold it into the per-model MeanVariance accumulators, reset."""
        row = self.sample_row()
        file.write("\t".join(("%.6f" % v) if k < 10 else ("%e" % v) for k, v in enumerate(row)) + "\n")
        file.flush()
        if self.n > 0:
            for c, v in zip(COLUMNS, row):
                self.clips[c].append(v)
        self.reset()
        return row

    def write_histogram(self, file):
        file.write("BinStart\tBinEnd\tL2ErrorMask\tCosineErrorNormal\tL2ErrorDepth\tL2ErrorAO\tL2ErrorColorWithAO\tL2ErrorColorNoAO\n")
        if self.metrics == "hip":
            self.histograms = dict(zip(self.histograms, self._dev_histograms.cpu().numpy()))
        hs = self.histograms
        for i in range(NUM_BINS):
            file.write("%7.5f\t%7.5f\t%e\t%e\t%e\t%e\t%e\t%e\n" % (i / NUM_BINS, (i + 1) / NUM_BINS, hs["mask"][i], hs["normal"][i],
                                                                  hs["depth"][i], hs["ao"][i], hs["color_withAO"][i], hs["color_noAO"][i]))


def clip_files(folder):
    """(low, high, flow) paths of the consecutively numbered clips of ``folder`` (``:312-318``)."""
    out = []
    for i in range(10000):
        low = os.path.join(folder, "low_%05d.npy" % i)
        if not os.path.isfile(low):
            break
        out.append((low, os.path.join(folder, "high_%05d.npy" % i), os.path.join(folder, "flow_%05d.npy" % i)))
    return out


def load_models(specs, device, upscaling=UPSCALING):
    """specs: [{'name': .., 'path': checkpoint or None (name = nearest | bilinear | bicubic) or 'model': an nn.Module}]
    -> [(name, module)] (``:99-105``: ``inference.LoadedModel(path).model``)."""
    from .inference import LoadedModel
    out = []
    for m in specs:
        if m.get("model") is not None:
            net = m["model"].to(device).eval()
        elif m.get("path"):
            net = LoadedModel(m["path"], device, upscaling).model
        else:
            net = SimpleUpsample(upscaling, m["name"]).to(device)
        if not isinstance(net, SimpleUpsample) and getattr(net, "output_channels", 6) != 6:
            # the clips, the recurrence of run_clip and every column are those of the 6-channel unshaded networks (mainPSNR3_AllStats.py)
            raise NotImplementedError("stats: model '%s' has %d output channels; only the unshaded (mask / normal / depth / AO) networks "
                                      "are evaluated here, not the colour (RGB) ones" % (m["name"], net.output_channels))
        out.append((m["name"], net))
    return out


def _batch_of_one(clip):
    """[T, ...] -> [1, T, ...] as ``train.clip_recurrence`` takes a clip (a one-frame clip may come without flow)."""
    return clip[None] if clip is not None else None


def run_clip(net, low, high, flow, stats, upscaling=UPSCALING):
    """One clip through one model with the recurrence of ``:326-371``; returns the clip's row."""
    def forward(single_input):
        # (on the device: with the guard contract of LoadedModel.inference around the call -- poll, first-frame range check, publish;
        # run_statistics flushes the last frame's words at the end of the clip)
        return clamp_prediction(net(single_input)[0] if isinstance(net, SimpleUpsample) else guarded_forward(net, single_input))
    for frame in clip_recurrence(forward, low[None], _batch_of_one(flow), 6, upscale=upscaling):
        stats.add_timestep_sample(frame.output, high[frame.j:frame.j + 1], low[frame.j:frame.j + 1])
    return stats


def run_statistics(datasets, model_specs, output_folder, device="cuda", upscaling=UPSCALING, border=BORDER, min_filling=MIN_FILLING,
                   log=print, metric_dtype=torch.float64, metrics="torch"):
    """``datasets``: [(name, [folders])] (``:29-41``); ``model_specs``: see ``load_models``; ``metrics``: see ``Statistics``.  Writes ``Stats_<dataset>_<model>.txt``,
    ``Histogram_<dataset>_<model>.txt`` and ``Summary_<dataset>.txt`` into ``output_folder``; returns
    {dataset: {model: {column: (mean, variance, clips)}}}."""
    os.makedirs(output_folder, exist_ok=True)
    nets = load_models(model_specs, device, upscaling)
    is_cuda = str(device).startswith("cuda")
    result = {}
    for dataset_name, folders in datasets:
        log("Compute statistics for", dataset_name)
        files = [open(os.path.join(output_folder, "Stats_%s_%s.txt" % (dataset_name, name)), "w") for name, _ in nets]
        stats = [Statistics(device, upscaling=upscaling, border=border, min_filling=min_filling, metric_dtype=metric_dtype, metrics=metrics)
                 for _ in nets]
        try:
            for f in files:
                Statistics.write_header(f)
            with torch.no_grad():
                for folder in folders:
                    for p_low, p_high, p_flow in clip_files(folder):
                        low, high, flow = (torch.from_numpy(np.load(p)).to(device) for p in (p_low, p_high, p_flow))
                        for (name, net), st, f in zip(nets, stats, files):
                            st.reset()
                            if is_cuda:
                                from . import ops
                                # every (model, clip) starts like a freshly loaded model: guard words handed out anew, the clip's FIRST frame gets
                                # the synchronous range check (LoadedModel._setup does the same for a checkpoint) -- several models take turns here
                                ops.range_reset()
                            run_clip(net, low, high, flow, st, upscaling)
                            if is_cuda:
                                from . import ops
                                ops.guards_flush(device)           # the clip's last frame is looked at too
                            st.write_sample(f)
            for (name, _), st in zip(nets, stats):
                with open(os.path.join(output_folder, "Histogram_%s_%s.txt" % (dataset_name, name)), "w") as hf:
                    st.write_histogram(hf)
        finally:
            for f in files:
                f.close()
        result[dataset_name] = write_summary(os.path.join(output_folder, "Summary_%s.txt" % dataset_name), nets, stats, COLUMNS)
    return result


def write_summary(path, nets, stats, columns):
    """``Summary_<dataset>.txt``: mean and variance over the clips of every column, one line per model; returns the same as a dict."""
    summary = {name: {c: (st.clips[c].mean(), st.clips[c].var(), st.clips[c].count()) for c in columns} for (name, _), st in zip(nets, stats)}
    with open(path, "w") as sf:
        sf.write("model\tclips\t" + "\t".join("%s-mean\t%s-var" % (c, c) for c in columns) + "\n")
        for name, cols in summary.items():
            sf.write("%s\t%d\t" % (name, cols[columns[0]][2]) + "\t".join("%.6f\t%e" % (cols[c][0], cols[c][1]) for c in columns) + "\n")
    return summary


# ---- the colour table: SuperresolutionNetwork/mainPSNR4_ColoredNets.py ----

COLOUR_COLUMNS = ("PSNR-color", "SSIM-color")
COLOUR_OWN_CHANNELS = 8                 # what ShadedModel feeds: shaded RGB, mask in [0, 1], normal, depth (:156-160)


class BaselineColourModel:
    """``SimpleUpsample`` of ``:112-143``: the five input channels resized, AO = 1, clamped (``:138-140``), shaded.  Like the other two
    wrappers it takes a frame's input -- the five low-resolution channels, then the flattened warped previous image -- and returns
    (colour, the image to feed back)."""
    prev_input_channels = 6

    def __init__(self, upscaling, upsample, shading):
        self.resize, self.shading = SimpleUpsample(upscaling, upsample), shading

    def __call__(self, single_input):
        prediction = clamp_prediction(self.resize(single_input)[0])
        return self.shading(prediction), prediction


class UnshadedColourModel:
    """``UnshadedModel`` of ``:169-190``: an unshaded network, its clamped G-buffer (``:185-187``) shaded afterwards and fed back."""
    prev_input_channels = 6

    def __init__(self, net, shading):
        self.net, self.shading = net, shading

    def __call__(self, single_input):
        prediction = clamp_prediction(guarded_forward(self.net, single_input))
        return self.shading(prediction), prediction


class ShadedColourModel:
    """``ShadedModel`` of ``:145-167``: a colour network on ``shade(low) | mask in [0, 1] | normal | depth`` and the flattened previous
    colour; its clamped output is the colour AND what is fed back."""
    prev_input_channels = 3

    def __init__(self, net, shading):
        self.net, self.shading = net, shading

    def __call__(self, single_input):
        sample_low, previous_warped_flattened = single_input[:, 0:5], single_input[:, 5:]
        own = torch.cat([self.shading(sample_low), sample_low[:, 0:1] * 0.5 + 0.5, sample_low[:, 1:4], sample_low[:, 4:5]], dim=1)
        color = torch.clamp(guarded_forward(self.net, torch.cat((own, previous_warped_flattened), dim=1)), 0, 1)
        return color, color


def load_colour_models(specs, device, shading, upscaling=UPSCALING):
    """specs as ``load_models`` -> [(name, wrapper)] (``:192-202``): checkpoints (and in-memory networks) go through
    ``inference.LoadedModel``, whose ``unshaded`` chooses the wrapper.  A colour network must take the eight own channels the script
    feeds (``ValueError`` otherwise)."""
    from .inference import LoadedModel
    out = []
    for m in specs:
        if m.get("model") is None and not m.get("path"):
            out.append((m["name"], BaselineColourModel(upscaling, m["name"], shading)))
            continue
        lm = LoadedModel.from_model(m["model"], device, upscaling, name=m["name"]) if m.get("model") is not None \
            else LoadedModel(m["path"], device, upscaling)
        if lm.unshaded:
            out.append((m["name"], UnshadedColourModel(lm.model, shading)))
            continue
        expected = COLOUR_OWN_CHANNELS + 3 * upscaling ** 2
        if lm.input_channels != expected:
            raise ValueError("colour statistics: model '%s' takes %d input channels; the table feeds colour networks shaded RGB, mask, "
                             "normal and depth plus the previous colour frame, %d channels" % (m["name"], lm.input_channels, expected))
        out.append((m["name"], ShadedColourModel(lm.model, shading)))
    return out


class ColourStatistics:
    """``Statistics`` of ``mainPSNR4_ColoredNets.py:215-280``: masked PSNR and MS-SSIM of the colour against the shaded ground truth,
    border cut off, sparsely covered frames skipped.  (The script's two histograms are allocated and never filled: none here.)
    ``metrics``: "torch" | "hip" as in ``Statistics``."""

    def __init__(self, device, shading, upscaling=UPSCALING, border=BORDER, min_filling=MIN_FILLING, metric_dtype=torch.float64,
                 metrics="torch"):
        check_metrics(metrics, device, metric_dtype)
        self.device, self.shading, self.metric_dtype, self.metrics = device, shading, metric_dtype, metrics
        self.upscaling, self.border, self.min_filling = upscaling, border, min_filling
        self.ssim = MSSSIM().to(device)
        self.psnr = PSNR().to(device)
        self.clips = {c: MeanVariance() for c in COLOUR_COLUMNS}
        self._windows = {}
        self.reset()

    def reset(self):
        self.n = 0
        self.sums = torch.zeros(2, dtype=torch.float64, device=self.device) if self.metrics == "hip" else [0.0, 0.0]

    @staticmethod
    def write_header(file):
        file.write("\t".join(COLOUR_COLUMNS) + "\n")

    def add_timestep_sample(self, pred_color, gt_mnda):
        """pred_color [1, 3, H, W]; gt_mnda [1, 6, H, W] (``:237-269``)."""
        gt_color = self.shading(gt_mnda)
        b2 = self.border * self.upscaling
        if b2 > 0:
            gt_mnda, pred_color, gt_color = (t[:, :, b2:-b2, b2:-b2] for t in (gt_mnda, pred_color, gt_color))
        md = self.metric_dtype
        if self.metrics == "hip":
            from . import ops
            mask = gt_mnda[0, 0].to(md) * 0.5 + 0.5
            H, W = mask.shape
        else:
            pred_color, gt_color = pred_color.to(md), gt_color.to(md)
            mask = gt_mnda[:, 0:1].to(md) * 0.5 + 0.5
            _, _, H, W = mask.shape
        if torch.sum(mask).item() / (H * W) < self.min_filling:
            return False
        self.n += 1
        if self.metrics == "hip":
            if (H, W) not in self._windows:
                self._windows[(H, W)] = ops.msssim_windows(H, W, self.device)
            pred_color, gt_color = pred_color.float(), gt_color.float()
            psnr = ops.psnr_from_sq_err(ops.masked_sq_err(pred_color, gt_color, mask), pred_color.shape[1], H, W, masked=True)
            self.sums = self.sums + torch.stack([psnr, ops.msssim_terms(pred_color, gt_color, windows=self._windows[(H, W)])[-1]])
        else:
            self.sums[0] += self.psnr(pred_color, gt_color, mask=mask).item()
            self.sums[1] += self.ssim(pred_color, gt_color).item()
        return True

    def sample_row(self):
        n = max(1, self.n)
        return [v / n for v in (self.sums.tolist() if self.metrics == "hip" else self.sums)]

    def write_sample(self, file):
        row = self.sample_row()
        file.write("%.6f\t%.6f\n" % tuple(row))
        file.flush()
        if self.n > 0:
            for c, v in zip(COLOUR_COLUMNS, row):
                self.clips[c].append(v)
        self.reset()
        return row


def run_colour_clip(model, low, high, flow, stats, upscaling=UPSCALING):
    """One clip through one wrapper with the recurrence of ``:314-346``: the previous image (6 or 3 channels, zeros on frame 0) is
    warped with ``special_mask=True`` -- for a three-channel previous COLOUR as well, whose red channel the reference thereby treats
    as a mask; kept."""
    for frame in clip_recurrence(model, low[None], _batch_of_one(flow), model.prev_input_channels, upscale=upscaling,
                                 feedback=lambda output: output[1]):                    # a wrapper returns (colour, the image to feed back)
        stats.add_timestep_sample(frame.output[0], high[frame.j:frame.j + 1])
    return stats


def run_colour_statistics(datasets, model_specs, output_folder, device="cuda", upscaling=UPSCALING, border=BORDER, min_filling=MIN_FILLING,
                          log=print, metric_dtype=torch.float64, metrics="auto"):
    """The colour table (``mainPSNR4_ColoredNets.py``): ``datasets`` / ``model_specs`` as ``run_statistics``, but the specs may name
    colour networks.  Writes ``Stats_<dataset>_<model>.txt`` (header ``PSNR-color  SSIM-color``, one row per clip) and
    ``Summary_<dataset>.txt``; returns {dataset: {model: {column: (mean, variance, clips)}}}.  ``metrics``: "auto" | "torch" | "hip"."""
    os.makedirs(output_folder, exist_ok=True)
    metrics = resolve_metrics(metrics, device, metric_dtype)
    shading = colour_shading(device)
    nets = load_colour_models(model_specs, device, shading, upscaling)
    is_cuda = str(device).startswith("cuda")
    result = {}
    for dataset_name, folders in datasets:
        log("Compute colour statistics for", dataset_name)
        files = [open(os.path.join(output_folder, "Stats_%s_%s.txt" % (dataset_name, name)), "w") for name, _ in nets]
        stats = [ColourStatistics(device, shading, upscaling, border, min_filling, metric_dtype, metrics) for _ in nets]
        try:
            for f in files:
                ColourStatistics.write_header(f)
            with torch.no_grad():
                for folder in folders:
                    for p_low, p_high, p_flow in clip_files(folder):
                        low, high, flow = (torch.from_numpy(np.load(p)).to(device) for p in (p_low, p_high, p_flow))
                        for (name, model), st, f in zip(nets, stats, files):
                            st.reset()
                            if is_cuda:
                                from . import ops
                                ops.range_reset()                  # as run_statistics: every (model, clip) starts like a freshly loaded model
                            run_colour_clip(model, low, high, flow, st, upscaling)
                            if is_cuda:
                                ops.guards_flush(device)
                            st.write_sample(f)
        finally:
            for f in files:
                f.close()
        result[dataset_name] = write_summary(os.path.join(output_folder, "Summary_%s.txt" % dataset_name), nets, stats, COLOUR_COLUMNS)
    return result


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="PSNR / MS-SSIM statistics of super-resolution models over clip folders (mainPSNR3_AllStats.py)")
    ap.add_argument("--dataset", action="append", required=True, help="name=folder[,folder...] (repeatable)")
    ap.add_argument("--model", action="append", default=[], help="name=checkpoint.pth (repeatable); nearest / bilinear / bicubic are always included")
    ap.add_argument("--output", default="results")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--table", choices=("unshaded", "colour"), default="unshaded",
                    help="unshaded: the 14 G-buffer columns (mainPSNR3_AllStats.py); colour: PSNR / MS-SSIM of the colour, colour networks included "
                         "(mainPSNR4_ColoredNets.py)")
    ap.add_argument("--metrics", choices=("torch", "hip"), default=None,
                    help="metric stage: the torch operations or the kernels of csrc/sr_metrics.hip (default: torch; colour table: the kernels "
                         "on a CUDA device)")
    args = ap.parse_args(argv)
    datasets = [(d.split("=", 1)[0], d.split("=", 1)[1].split(",")) for d in args.dataset]
    specs = [{"name": n, "path": None} for n in ("nearest", "bilinear", "bicubic")]
    specs += [{"name": m.split("=", 1)[0], "path": m.split("=", 1)[1]} for m in args.model]
    if args.table == "colour":
        res = run_colour_statistics(datasets, specs, args.output, device=args.device, metrics=args.metrics or "auto")
        for ds, per_model in res.items():
            for name, cols in per_model.items():
                print("%s / %s: PSNR-color %.3f dB, SSIM-color %.5f over %d clips" % (ds, name, cols["PSNR-color"][0], cols["SSIM-color"][0], cols["PSNR-color"][2]))
        return
    res = run_statistics(datasets, specs, args.output, device=args.device, metrics=args.metrics or "torch")
    for ds, per_model in res.items():
        for name, cols in per_model.items():
            print("%s / %s: PSNR-normal %.3f dB, SSIM-normal %.5f over %d clips" % (ds, name, cols["PSNR-normal"][0], cols["SSIM-normal"][0], cols["PSNR-normal"][2]))


if __name__ == "__main__":
    main()
