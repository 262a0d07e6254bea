// One wave64 = one 8 x 8 pixel tile: what every render kernel of both semantics (iso_kernels.hip, iso_gvdb.hip) does
// before and after its own work -- which tile, which pixel, is it on the image and inside the viewport, and the store.
#pragma once
#include <hip/hip_runtime.h>

#include "iso_params.h"

// XCD-aware tile order: blocks b and b+8 share an XCD/L2, so give each XCD a contiguous run of
// tiles (neighbouring pixel tiles walk the same bricks).  Bijective for any tile count.
__device__ __forceinline__ int xcd_remap(int bid, int nwg)
{
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// pixel (i, j) of lane `lane` of raster tile `tile`; a ragged tile has lanes off the image, which must not store
struct TilePixel { int i, j; bool in_image, inside; };
__device__ __forceinline__ TilePixel tile_pixel(const IsoRenderParams& P, int tile, int lane)
{
    const int tiles_x = iso_tiles_x(P.W);
    TilePixel t;
    t.i = (tile % tiles_x) * 8 + (lane & 7);
    t.j = (tile / tiles_x) * 8 + (lane >> 3);
    t.in_image = t.i < P.W && t.j < P.H;
    t.inside = t.in_image && t.i >= P.vp[0] && t.j >= P.vp[1] && t.i < P.vp[2] && t.j < P.vp[3];
    return t;
}

__device__ __forceinline__ void store_pixel(const IsoRenderParams& P, int i, int j, const float o[12])
{
    float4* dst = reinterpret_cast<float4*>(P.out + ((size_t)j * P.W + i) * 12);
    dst[0] = make_float4(o[0], o[1], o[2], o[3]);
    dst[1] = make_float4(o[4], o[5], o[6], o[7]);
    dst[2] = make_float4(o[8], o[9], o[10], o[11]);
}
