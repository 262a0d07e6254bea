// Brick store, range tables and march flags of the ray-marcher: the kernels that turn a dense volume (or a sparse brick
// list) into what iso_kernels.hip and iso_gvdb.hip traverse, and their launchers.  They share nothing with the traversal
// but the parameter header.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iso_params.h"

namespace {

// Per-leaf / per-node flags for the frame's isovalue (iso_march_flags, refreshed by the host whenever the isovalue or the
// volume changes): bit 0 = the leaf / node exists, bit 1 = it exists and must be marched.
// In a tile, P.leaf holds "leaf exists AND is owned by this tile": leaves of the halo are walked past like empty space.
// Min/max skipping, exact: every sample the voxel DDA of a leaf can take reads voxels of [8b-1, 8b+9]^3 only (cells
// 8b-1 .. 8b+8: a position may sit a rounding error outside the leaf's faces), and a trilinear value stays inside the
// range of its 8 corners up to ~11 ulp of the seven float lerps.  If the isovalue lies outside [min, max] of that
// neighbourhood by more than the pad, (value - iso) has one strict sign along the whole march, the reference's
// `v0 * v1 <= 0` never fires, and stepping over the leaf is the same computation.  Long rays that cross the thin
// low-density fringe or the dense core without meeting the surface were the tail the whole frame waited for.
// The same one level up: node1Range = (min, max) over the ranges of the node's existing leaves.  If the isovalue lies
// outside it, no leaf of the node can be marched, and since the leaf-level DDA is re-initialised per node
// (IsoVolumeRayTracer.h:37-46) stepping over the whole node changes nothing downstream.
__device__ __forceinline__ bool range_may_cross(const float* mm, double iso)
{
    const double lo = (double)mm[0], hi = (double)mm[1];
    const double pad = 4e-6 * fmax(fabs(lo), fabs(hi));
    return !(iso < lo - pad || iso > hi + pad);
}

__global__ __launch_bounds__(256) void iso_march_flags(const uint8_t* __restrict__ exists, const float* __restrict__ range, int n, double iso,
                                                       uint8_t* __restrict__ flags)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = exists[i] ? (uint8_t)(1 | (range_may_cross(range + 2 * (size_t)i, iso) ? 2 : 0)) : (uint8_t)0;
}

// ---- brick builder -------------------------------------------------------------------------
// One 64-lane workgroup per 8^3 brick position.  flag9: any non-zero among the 9^3 apron values
// (brick must be stored); leaf: any non-zero among the 8^3 own voxels (OpenVDB leaf exists);
// bbox6 / maxbits: active-voxel bbox and maximum (grid->evalMinMax, CPURenderer.cpp:501-502).
__device__ __forceinline__ unsigned int float_order_bits(float f)
{
    unsigned int u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(64) void iso_brick_flags(const float* __restrict__ dense, int nx, int ny, int nz,
                                                     int nbx, int nby, int nbz,
                                                     uint8_t* flag9, uint8_t* leaf, int* bbox6, unsigned int* maxbits)
{
    const int b = blockIdx.x;
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    const int lane = threadIdx.x;
    bool any9 = false, any8 = false;
    int mnx = INT32_MAX, mny = INT32_MAX, mnz = INT32_MAX, mxx = INT32_MIN, mxy = INT32_MIN, mxz = INT32_MIN;
    unsigned int mb = 0;
    for (int k = lane; k < ISO_BRICK_VALUES; k += 64) {
        const int lx = k % 9, ly = (k / 9) % 9, lz = k / 81;
        const int x = bx * 8 + lx, y = by * 8 + ly, z = bz * 8 + lz;
        float f = 0.0f;
        if (x < nx && y < ny && z < nz) f = dense[((size_t)z * ny + y) * nx + x];
        if (f != 0.0f) {
            any9 = true;
            if (lx < 8 && ly < 8 && lz < 8) {
                any8 = true;
                mnx = min(mnx, x); mny = min(mny, y); mnz = min(mnz, z);
                mxx = max(mxx, x); mxy = max(mxy, y); mxz = max(mxz, z);
                mb = max(mb, float_order_bits(f));
            }
        }
    }
    const unsigned long long m9 = __ballot(any9), m8 = __ballot(any8);
    if (m8) {
        for (int off = 32; off > 0; off >>= 1) {
            mnx = min(mnx, __shfl_xor(mnx, off)); mny = min(mny, __shfl_xor(mny, off)); mnz = min(mnz, __shfl_xor(mnz, off));
            mxx = max(mxx, __shfl_xor(mxx, off)); mxy = max(mxy, __shfl_xor(mxy, off)); mxz = max(mxz, __shfl_xor(mxz, off));
            mb = max(mb, (unsigned int)__shfl_xor((int)mb, off));
        }
    }
    if (lane == 0) {
        flag9[b] = m9 ? 1 : 0;
        leaf[b] = m8 ? 1 : 0;
        if (m8) {
            atomicMin(&bbox6[0], mnx); atomicMin(&bbox6[1], mny); atomicMin(&bbox6[2], mnz);
            atomicMax(&bbox6[3], mxx); atomicMax(&bbox6[4], mxy); atomicMax(&bbox6[5], mxz);
            atomicMax(maxbits, mb);
        }
    }
}

__global__ __launch_bounds__(64) void iso_brick_fill(const float* __restrict__ dense, int nx, int ny, int nz,
                                                    int nbx, int nby, int nbz,
                                                    const int32_t* __restrict__ slot, float* __restrict__ bricks)
{
    const int b = blockIdx.x;
    const int s = slot[b];
    if (s < 0) return;
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    float* dst = bricks + (size_t)s * ISO_BRICK_STRIDE;
    for (int k = threadIdx.x; k < ISO_BRICK_STRIDE; k += 64) {
        float f = 0.0f;
        if (k < ISO_BRICK_VALUES) {
            const int lx = k % 9, ly = (k / 9) % 9, lz = k / 81;
            const int x = bx * 8 + lx, y = by * 8 + ly, z = bz * 8 + lz;
            if (x < nx && y < ny && z < nz) f = dense[((size_t)z * ny + y) * nx + x];
        }
        dst[k] = f;
    }
}

// range[b] = (min, max) over the voxels [8b-1, 8b+9]^3 of brick position b; outside the grid counts as 0
__global__ __launch_bounds__(64) void iso_leaf_range(const float* __restrict__ dense, int nx, int ny, int nz,
                                                    int nbx, int nby, int nbz, float* __restrict__ range)
{
    const int b = blockIdx.x;
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    float lo = 3.0e38f, hi = -3.0e38f;
    for (int k = threadIdx.x; k < 11 * 11 * 11; k += 64) {
        const int lx = k % 11, ly = (k / 11) % 11, lz = k / 121;
        const int x = bx * 8 - 1 + lx, y = by * 8 - 1 + ly, z = bz * 8 - 1 + lz;
        float f = 0.0f;
        if ((unsigned)x < (unsigned)nx && (unsigned)y < (unsigned)ny && (unsigned)z < (unsigned)nz) f = dense[((size_t)z * ny + y) * nx + x];
        lo = fminf(lo, f); hi = fmaxf(hi, f);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off));
        hi = fmaxf(hi, __shfl_xor(hi, off));
    }
    if (threadIdx.x == 0) { range[2 * (size_t)b] = lo; range[2 * (size_t)b + 1] = hi; }
}

// nodeRange[n] = (min of the leaf minima, max of the leaf maxima) over the existing leaves of 128^3 node n
__global__ __launch_bounds__(64) void iso_node_range(const uint8_t* __restrict__ leaf, const float* __restrict__ leafRange,
                                                    int nbx, int nby, int nbz, int ox, int oy, int oz, int n1x, int n1y, int n1ox, int n1oy, int n1oz,
                                                    float* __restrict__ nodeRange)
{
    const int n = blockIdx.x;
    const int ax = n % n1x, ay = (n / n1x) % n1y, az = n / (n1x * n1y);
    float lo = 3.0e38f, hi = -3.0e38f;
    for (int k = threadIdx.x; k < 4096; k += 64) {
        // global brick coordinates of the node's k-th leaf position, then local to the stored region
        const int bx = ((ax + n1ox) << 4) + (k & 15) - (ox >> 3), by = ((ay + n1oy) << 4) + ((k >> 4) & 15) - (oy >> 3),
                  bz = ((az + n1oz) << 4) + (k >> 8) - (oz >> 3);
        if ((unsigned)bx >= (unsigned)nbx || (unsigned)by >= (unsigned)nby || (unsigned)bz >= (unsigned)nbz) continue;
        const size_t b = ((size_t)bz * nby + by) * nbx + bx;
        if (!leaf[b]) continue;
        lo = fminf(lo, leafRange[2 * b]); hi = fmaxf(hi, leafRange[2 * b + 1]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off));
        hi = fmaxf(hi, __shfl_xor(hi, off));
    }
    if (threadIdx.x == 0) { nodeRange[2 * (size_t)n] = lo; nodeRange[2 * (size_t)n + 1] = hi; }
}

// sparse loads (.vbx brick lists): the tables of the few existing positions are scattered into memset tables
__global__ __launch_bounds__(256) void iso_scatter_tables(int n, const long long* __restrict__ index, const int32_t* __restrict__ slotv,
                                                         const uint8_t* __restrict__ leafv, const float* __restrict__ rangev,
                                                         int32_t* __restrict__ slot, uint8_t* __restrict__ leaf, float* __restrict__ range)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long b = index[i];
    slot[b] = slotv[i];
    leaf[b] = leafv[i];
    range[2 * b] = rangev[2 * i];
    range[2 * b + 1] = rangev[2 * i + 1];
}

}  // namespace

void iso_launch_node_range(const uint8_t* leaf, const float* leafRange, int nbx, int nby, int nbz, const int org[3],
                           int n1x, int n1y, int n1z, const int n1o[3], float* nodeRange, void* stream)
{
    hipLaunchKernelGGL(iso_node_range, dim3(n1x * n1y * n1z), dim3(64), 0, (hipStream_t)stream, leaf, leafRange, nbx, nby, nbz,
                       org[0], org[1], org[2], n1x, n1y, n1o[0], n1o[1], n1o[2], nodeRange);
}

void iso_launch_scatter_tables(int n, const long long* index, const int32_t* slotv, const uint8_t* leafv, const float* rangev,
                               int32_t* slot, uint8_t* leaf, float* range, void* stream)
{
    if (n > 0)
        hipLaunchKernelGGL(iso_scatter_tables, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, index, slotv, leafv, rangev, slot, leaf, range);
}

void iso_launch_leaf_range(const float* dense, int nx, int ny, int nz, int nbx, int nby, int nbz, float* range, void* stream)
{
    hipLaunchKernelGGL(iso_leaf_range, dim3(nbx * nby * nbz), dim3(64), 0, (hipStream_t)stream, dense, nx, ny, nz, nbx, nby, nbz, range);
}

void iso_launch_march_flags(const uint8_t* exists, const float* range, int n, double iso, uint8_t* flags, void* stream)
{
    if (n > 0) hipLaunchKernelGGL(iso_march_flags, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, exists, range, n, iso, flags);
}

void iso_launch_brick_flags(const float* dense, int nx, int ny, int nz, int nbx, int nby, int nbz,
                            uint8_t* flag9, uint8_t* leaf, int* bbox6, unsigned int* maxbits, void* stream)
{
    hipLaunchKernelGGL(iso_brick_flags, dim3(nbx * nby * nbz), dim3(64), 0, (hipStream_t)stream,
                       dense, nx, ny, nz, nbx, nby, nbz, flag9, leaf, bbox6, maxbits);
}

void iso_launch_brick_fill(const float* dense, int nx, int ny, int nz, int nbx, int nby, int nbz,
                           const int32_t* slot, float* bricks, void* stream)
{
    hipLaunchKernelGGL(iso_brick_fill, dim3(nbx * nby * nbz), dim3(64), 0, (hipStream_t)stream,
                       dense, nx, ny, nz, nbx, nby, nbz, slot, bricks);
}
