"""One-off A/B of the weight-gradient host path: the parent commit's product library (tools/build_head_lib.sh -> tools/lib_head/) and this
tree's, loaded side by side in ONE process, on shapes on either side of every rule of wgrad_plan (csrc/sr_wgrad.hip).  The forms of one
kind differ in slab count and therefore in summation order, so `torch.equal` of dw / db pins the plan.  Also: the validation's return
codes on both libraries, and the parent's armed accumulate against this tree's argument.  Prints a markdown table (profiles/wgrad_tu_ab.md).

    PYTHONPATH=. python tools/lab/wgrad_tu_ab.py [--parent tools/lib_head/libisr_sr.so]
"""
import argparse
import ctypes
import os
import sys

import torch

from isosurfacesuperresolution_amd import _native, ops

vp, ci = ctypes.c_void_p, ctypes.c_int
SEG = [vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp]
MAX_OLD = [vp, vp, vp, ci, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp]
MAX_NEW = [vp, vp, vp, ci, ci, vp, vp, ci, vp, ci, ci, ci, ci, ci, vp]


def bind(path, new):
    lib = ctypes.CDLL(path)
    for name in ("isrConv3x3WeightGradSegments", "isrConv3x3WeightGradSegmentsBf16", "isrConv3x3WeightGradSegmentsSplit"):
        getattr(lib, name).argtypes = SEG
        getattr(lib, name).restype = ci
    lib.isrConv3x3WeightGradSegmentsSplitMax.argtypes = MAX_NEW if new else MAX_OLD
    lib.isrConv3x3WeightGradSegmentsSplitMax.restype = ci
    lib.isrConvWeightGradWorkspace.argtypes = [ci] * 5
    lib.isrConvWeightGradWorkspace.restype = ctypes.c_longlong
    if not new:
        lib.isrSetWeightGradAccumulate.argtypes = [ci]
        lib.isrSetWeightGradAccumulate.restype = None
    return lib


def ptrs(ts):
    return (vp * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def call(lib, new, kind, xs, gzs, gzmax, dw, db, ws, shape, accumulate=0, segments=None):
    n, cin, h, w, cout = shape
    segs = len(xs) if segments is None else segments
    tail = (ops._ptr(ws), n, cin, h, w, cout, None)
    if kind == "split":
        pm = ptrs(gzmax) if gzmax is not None else None
        if new:
            rc = lib.isrConv3x3WeightGradSegmentsSplitMax(ptrs(xs), ptrs(gzs), pm, 1 if gzmax else 0, segs, ops._ptr(dw), ops._ptr(db), accumulate, *tail)
        else:
            if accumulate:
                lib.isrSetWeightGradAccumulate(accumulate)
            rc = lib.isrConv3x3WeightGradSegmentsSplitMax(ptrs(xs), ptrs(gzs), pm, 1 if gzmax else 0, segs, ops._ptr(dw), ops._ptr(db), *tail)
    else:
        fn = lib.isrConv3x3WeightGradSegmentsBf16 if kind == "bf16" else lib.isrConv3x3WeightGradSegments
        rc = fn(ptrs(xs), ptrs(gzs), segs, ops._ptr(dw), ops._ptr(db), *tail)
    torch.cuda.synchronize()
    return rc


def pairs(segs, n, cin, cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.relu(torch.randn(n, cin, h, w, generator=g)).cuda() for _ in range(segs)]
    gzs = [(torch.randn(n, cout, h, w, generator=g) * 1e-2).cuda() for _ in range(segs)]
    return xs, gzs


def plan_cases():
    """(kind, tiles, cin, cout, with gzmax, what the case straddles); one 4 x 32 tile per image, so tiles = segments x N"""
    out = []
    for nt in (191, 192, 193):
        out.append(("exact", nt, 64, 64, False, "G <= 192: three workgroups per tile set"))
    for kind in ("exact", "bf16", "split"):
        for nt in (511, 512, 1023, 1024):
            out.append((kind, nt, 64, 64, False, "many tiles: G = 256 from %d on" % (1024 if kind == "exact" else 512)))
    for nt in (256, 257):
        for cout in (32, 33):
            out.append(("exact", nt, 64, cout, False, "KSPLIT: <= 32 channels left and G <= 256"))
    out.append(("exact", 1024, 64, 96, False, "KSPLIT on the last channel block only (G = 256)"))
    for kind in ("exact", "bf16", "split"):
        for cin in (6, 64, 128):
            for cout in (6, 64, 128):
                out.append((kind, 300, cin, cout, False, "co0 / ci0 loop, bias slabs on ci0 == 0"))
    for nt, cin, cout in ((300, 64, 64), (512, 64, 64), (300, 128, 128), (300, 6, 6), (1024, 64, 6)):
        out.append(("split", nt, cin, cout, True, "scale from the producers' maxima"))
    return out


def segments_of(nt):
    for s in (4, 3, 2):
        if nt % s == 0:
            return s
    return 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lib_head", "libisr_sr.so"))
    args = ap.parse_args()
    libs = {"parent": bind(os.path.abspath(args.parent), False), "new": bind(os.path.join(_native.LIBDIR, "libisr_sr.so"), True)}
    ws = torch.empty(libs["new"].isrConvWeightGradWorkspace(1, 64, 4, 32, 64), dtype=torch.uint8, device="cuda")
    assert libs["parent"].isrConvWeightGradWorkspace(1, 64, 4, 32, 64) == ws.numel()
    bad = 0
    print("## Routing: dw / db of the parent's library and this tree's, `torch.equal`\n")
    print("| kind | tiles | segments x N | Cin | Cout | gzmax | straddles | dw | db |")
    print("|---|---|---|---|---|---|---|---|---|")
    h, w = 4, 32
    for k, (kind, nt, cin, cout, tagged, why) in enumerate(plan_cases()):
        segs = segments_of(nt)
        n = nt // segs
        shape = (n, cin, h, w, cout)
        xs, gzs = pairs(segs, n, cin, cout, h, w, 1000 + k)
        gzmax = [t.abs().max().reshape(1).view(torch.int32) for t in gzs] if tagged else None
        res = {}
        for name, lib in libs.items():
            dw, db = torch.full((cout, cin, 3, 3), 7.0).cuda(), torch.full((cout,), 7.0).cuda()
            rc = call(lib, name == "new", kind, xs, gzs, gzmax, dw, db, ws, shape)
            assert rc == 0, (name, kind, nt, rc)
            res[name] = (dw, db)
        ew, eb = torch.equal(res["parent"][0], res["new"][0]), torch.equal(res["parent"][1], res["new"][1])
        live = res["new"][0].abs().max().item() > 0 and not res["new"][0].eq(7.0).any().item()
        bad += not (ew and eb and live)
        print("| %s | %d | %d x %d | %d | %d | %s | %s | %s | %s |" % (kind, nt, segs, n, cin, cout, "yes" if tagged else "no", why,
              "equal" if ew and live else "DIFFERS", "equal" if eb else "DIFFERS"))
        sys.stdout.flush()

    print("\n## Accumulate: the parent's armed setter against the argument (split kind, 300 tiles, 64 -> 64)\n")
    print("| bits | dw | db |")
    print("|---|---|---|")
    xs, gzs = pairs(3, 100, 64, 64, h, w, 77)
    g = torch.Generator().manual_seed(78)
    pre_w, pre_b = (torch.rand(64, 64, 3, 3, generator=g) - 0.5).cuda(), (torch.rand(64, generator=g) - 0.5).cuda()
    for bits in (0, 1, 2, 3):
        res = {}
        for name, lib in libs.items():
            dw, db = pre_w.clone(), pre_b.clone()
            assert call(lib, name == "new", "split", xs, gzs, None, dw, db, ws, (100, 64, h, w, 64), bits) == 0
            res[name] = (dw, db)
        ew, eb = torch.equal(res["parent"][0], res["new"][0]), torch.equal(res["parent"][1], res["new"][1])
        bad += not (ew and eb)
        print("| %d | %s | %s |" % (bits, "equal" if ew else "DIFFERS", "equal" if eb else "DIFFERS"))

    print("\n## Return codes of the validation (N = 1, 12 -> 6 channels, 5 x 36 pixels, two segments)\n")
    print("| entry | library | segments = 0 | segments = 33 | NULL pair | gzs[0] + 4 bytes | W = 6 |")
    print("|---|---|---|---|---|---|---|")
    n, cin, cout, hh, ww = 1, 12, 6, 5, 36
    xs, gzs = pairs(2, n, cin, cout, hh, ww, 5)
    xs6, gzs6 = pairs(2, n, cin, cout, hh, 6, 6)
    room = torch.zeros(gzs[0].numel() + 4, device="cuda")
    shifted = room[1:1 + gzs[0].numel()].view_as(gzs[0])
    shifted.copy_(gzs[0])
    assert shifted.data_ptr() % 16 == 4
    dw, db = torch.zeros(cout, cin, 3, 3).cuda(), torch.zeros(cout).cuda()
    for kind in ("exact", "bf16", "split"):
        rows = {}
        for name, lib in libs.items():
            new = name == "new"
            rows[name] = (call(lib, new, kind, xs, gzs, None, dw, db, ws, (n, cin, hh, ww, cout), segments=0),
                          call(lib, new, kind, xs * 17, gzs * 17, None, dw, db, ws, (n, cin, hh, ww, cout), segments=33),
                          call(lib, new, kind, [xs[0], None], gzs, None, dw, db, ws, (n, cin, hh, ww, cout)),
                          call(lib, new, kind, xs, [shifted, gzs[1]], None, dw, db, ws, (n, cin, hh, ww, cout)),
                          call(lib, new, kind, xs6, gzs6, None, dw, db, ws, (n, cin, hh, 6, cout)))
            print("| %s | %s | %d | %d | %d | %d | %d |" % ((kind, name) + rows[name]))
        bad += rows["parent"] != rows["new"]
    print("\n%s" % ("all equal" if not bad else "%d MISMATCHES" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
