// layout.hip -- volume layout conversions (canonical <-> bricked <-> paired) and the sparse gradient flush, with their
// C-ABI entry points
#include "diffus_host.hpp"

namespace {

// ----------------------------------------------------------------------------
// canonical <-> bricked conversion.  A block moves 4 x 4 x 64 voxels (32 bricks,
// 4 KiB): 16 canonical rows of 256 B on one side, 4 KiB contiguous on the other,
// through an LDS transpose so that both sides are coalesced.
constexpr int kConvZ = 64, kConvZThin = 8; // depths per block: whole volumes / thin sub-boxes (diffus_convert_volume_box)
template <bool TO_BRICKED, bool ACCUMULATE, int CZ = kConvZ>
__global__ __launch_bounds__(kBlock) void brick_convert_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                               Geom G, int zblk0 = 0, int by_0 = 0, int bx_0 = 0)
{
    __shared__ float t[16][CZ + 1];
    // (zblk0, by_0, bx_0): the first block of a sub-box conversion (diffus_convert_volume_box); 0 for a whole volume
    const int bz0 = ((int)blockIdx.x + zblk0) * (CZ / 2); // first brick along dim 2
    const int by = blockIdx.y + by_0, bx = blockIdx.z + bx_0;
    const int tid = threadIdx.x;
    const long brick0 = ((long)bx * G.nb1 + by) * G.nb2 + bz0;
    if (TO_BRICKED) {
        for (int e = tid; e < 16 * CZ; e += kBlock) {
            int row = e / CZ, zz = e - row * CZ;
            int x = bx * 4 + (row >> 2), y = by * 4 + (row & 3), z = bz0 * 2 + zz;
            t[row][zz] = (x < G.d0 && y < G.d1 && z < G.d2) ? in[((long)x * G.d1 + y) * G.d2 + z] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < 16 * CZ; e += kBlock) {
            int brick = e >> 5, off = e & 31;
            if (bz0 + brick < G.nb2) out[(brick0 + brick) * kBrickFloats + off] = t[off >> 1][brick * 2 + (off & 1)];
        }
    } else {
        for (int e = tid; e < 16 * CZ; e += kBlock) {
            int brick = e >> 5, off = e & 31;
            if (bz0 + brick < G.nb2) t[off >> 1][brick * 2 + (off & 1)] = in[(brick0 + brick) * kBrickFloats + off];
        }
        __syncthreads();
        for (int e = tid; e < 16 * CZ; e += kBlock) {
            int row = e / CZ, zz = e - row * CZ;
            int x = bx * 4 + (row >> 2), y = by * 4 + (row & 3), z = bz0 * 2 + zz;
            if (x < G.d0 && y < G.d1 && z < G.d2) {
                long o = ((long)x * G.d1 + y) * G.d2 + z;
                if (ACCUMULATE)
                    out[o] += t[row][zz];
                else
                    out[o] = t[row][zz];
            }
        }
    }
}

// Bricked gradient scratch -> canonical tensor.  Every touched brick (flag != 0) is added into (or stored to) the
// canonical tensor, ZEROED in the bricked buffer and its flag cleared, so the bricked buffer and the flags are all-zero
// again afterwards.  A fan touches a few thousand of the 524 288 bricks of a 256^3 volume: this replaces a 64 MiB memset
// plus a 128 MiB dense conversion per step.
// mode DIFFUS_FLUSH_PERSISTENT: `out` is a gradient tensor the caller keeps across steps and only this call writes.
// A brick stored this step gets flag 2 ("out holds last step's values, scratch is zero"); if the next step does not
// touch it again (the scatter overwrites the flag with 1) its voxels are zeroed in `out` and the flag cleared.  `out`
// therefore always equals the dense gradient of the latest step without ever being memset.
// mode DIFFUS_FLUSH_DENSE (this kernel): every voxel of `out` is written, one lane per brick.
__global__ __launch_bounds__(kBlock) void gradbuf_flush_dense_kernel(float *__restrict__ bricked, int *__restrict__ touched,
                                                                     float *__restrict__ out, Geom G, long nbricks)
{
    const int wib = threadIdx.x >> 6;
    const long w = (long)blockIdx.x * kWavesPerBlock + wib;
    const int lane = threadIdx.x & 63;
    const long b0 = w * kWave;
    if (b0 >= nbricks) return;
    const long mine = b0 + lane;
    int f = (mine < nbricks) ? touched[mine] : 0;
    {
        // EVERY voxel of `out` is written: a lane takes one brick, the wave 64 consecutive ones -- consecutive along dim 2,
        // so that each of a brick's 16 (x, y) rows is a 512-byte run of the canonical tensor across the wave.
        if (mine >= nbricks) return;
        if (f) touched[mine] = 0;
        const bool live = f == 1; // 2 = left by a PERSISTENT flush: the scratch is already zero there
        const unsigned um = (unsigned)mine, t = um / (unsigned)G.nb2, bz = um - t * (unsigned)G.nb2;
        const unsigned bx = t / (unsigned)G.nb1, by = t - bx * (unsigned)G.nb1;
        float *bsrc = bricked + mine * kBrickFloats;
        const int z = (int)bz * 2;
#pragma unroll 4
        for (int row = 0; row < 16; ++row) {
            const int x = (int)bx * 4 + (row >> 2), y = (int)by * 4 + (row & 3);
            float2 v = make_float2(0.f, 0.f);
            if (live) {
                v = *reinterpret_cast<const float2 *>(bsrc + row * 2);
                *reinterpret_cast<float2 *>(bsrc + row * 2) = make_float2(0.f, 0.f);
            }
            if (x < G.d0 && y < G.d1) {
                float *o = out + ((long)x * G.d1 + y) * G.d2 + z;
                if (z + 1 < G.d2 && !(G.d2 & 1)) {
                    *reinterpret_cast<float2 *>(o) = v;
                } else {
                    o[0] = v.x;
                    if (z + 1 < G.d2) o[1] = v.y;
                }
            }
        }
        return;
    }
}

// The sparse modes.  A wave reads the flags of 256 consecutive bricks (four coalesced loads), compacts the ids of the
// touched ones into LDS and walks them EIGHT per trip: 8 lanes per brick, a lane moving four floats = the z pairs of two
// neighbouring (x, y) rows.  (Rounds 2-3: 64 bricks per wave, two per trip -- 2048 blocks whose launch and flag reads were
// most of the kernel at 32 poses; 256 bricks per wave at two per trip was slower there, the serial walk four times longer.)
constexpr int kFlushBricks = 256;
template <bool VEC2> // VEC2: d2 even and `out` 8-byte aligned -- a z pair is one aligned 8-byte word of the canonical tensor
__global__ __launch_bounds__(kBlock) void gradbuf_flush_kernel(float *__restrict__ bricked, int *__restrict__ touched,
                                                               float *__restrict__ out, Geom G, long nbricks, int mode)
{
    __shared__ short s_list[kWavesPerBlock][kFlushBricks];
    const int wib = threadIdx.x >> 6;
    const long w = (long)blockIdx.x * kWavesPerBlock + wib;
    const int lane = threadIdx.x & 63;
    const long b0 = w * kFlushBricks;
    if (b0 >= nbricks) return;
    int f[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const long mine = b0 + c * kWave + lane;
        f[c] = (mine < nbricks) ? touched[mine] : 0;
    }
    if (__ballot((f[0] | f[1] | f[2] | f[3]) != 0) == 0ull) return; // wave-uniform: nothing touched in these 256 bricks
    int cnt = 0;
    const unsigned long long below = (1ull << lane) - 1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned long long m = __ballot(f[c] != 0);
        if (f[c]) {
            touched[b0 + c * kWave + lane] = (mode == DIFFUS_FLUSH_PERSISTENT && f[c] == 1) ? 2 : 0;
            // bit 8 marks a stale brick (nothing new this step: clear what the last step left in `out`)
            s_list[wib][cnt + __builtin_popcountll(m & below)] = (short)((c * kWave + lane) | (f[c] == 2 ? 256 : 0));
        }
        cnt += __builtin_popcountll(m);
    }
    wave_lds_sync();
    const int sub = lane & 7, grp = lane >> 3;
    // the lane's two rows inside a brick: x = sub / 2, y = 2 (sub % 2) and the next one; floats 4 sub .. 4 sub + 3
    const int xl = sub >> 1, yl = (sub & 1) * 2;
#pragma unroll 2
    for (int i = grp; i < cnt; i += 8) { // trips are independent: their loads overlap
        const int e = s_list[wib][i];
        const long brick = b0 + (e & 255);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!(e & 256)) { // uniform over the brick's 8 lanes
            float4 *src = reinterpret_cast<float4 *>(bricked + brick * kBrickFloats + sub * 4);
            v = *src;
            *src = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        // 32-bit index arithmetic (a volume has fewer than 2^25 bricks)
        const unsigned ub = (unsigned)brick, t = ub / (unsigned)G.nb2, bz = ub - t * (unsigned)G.nb2;
        const unsigned bx = t / (unsigned)G.nb1, by = t - bx * (unsigned)G.nb1;
        const int x = (int)bx * 4 + xl, y = (int)by * 4 + yl, z = (int)bz * 2;
        if (x >= G.d0) continue;
        float *o = out + ((long)x * G.d1 + y) * G.d2 + z;
#pragma unroll
        for (int r = 0; r < 2; ++r, o += G.d2) {
            if (y + r >= G.d1) break;
            const float v0 = r ? v.z : v.x, v1 = r ? v.w : v.y;
            if (VEC2) { // z + 1 < d2 always: d2 is even
                float2 *o2 = reinterpret_cast<float2 *>(o);
                if (mode == DIFFUS_FLUSH_ACCUMULATE) {
                    const float2 q = *o2;
                    *o2 = make_float2(q.x + v0, q.y + v1);
                } else {
                    *o2 = make_float2(v0, v1);
                }
            } else {
                o[0] = (mode == DIFFUS_FLUSH_ACCUMULATE) ? o[0] + v0 : v0;
                if (z + 1 < G.d2) o[1] = (mode == DIFFUS_FLUSH_ACCUMULATE) ? o[1] + v1 : v1;
            }
        }
    }
}

// canonical -> PAIRED: a block writes the records of TWO neighbouring 4 x 4 column blocks for 128 depths (two runs of
// 128 x 160 B) from 4 x 9 canonical rows of 129 floats (the ninth column and the 129th depth are the neighbours the
// records repeat, clamped at the volume's edge), through LDS so that both sides are coalesced: 512-byte row reads,
// 16-byte stores.  256^3: 42 us = 5.5 TB/s of (volume read + records written).  (First version: one column block x 32
// depths per block, 132-byte row reads, a quarter of them the halo column: the L2-side fetch was 1.9x the volume and
// the kernel took 80 us; 64 depths per block: 46 us.)
#ifndef DIFFUS_PC_Z
#define DIFFUS_PC_Z 128
#endif
constexpr int kPcZ = DIFFUS_PC_Z, kPcZThin = 8, kPcCols = 9, kPcRows = 4 * kPcCols; // kPcZThin: thin sub-boxes (diffus_convert_volume_box)
template <int PZ = kPcZ>
__global__ __launch_bounds__(kBlock) void pair_convert_kernel(const float *__restrict__ in, float *__restrict__ out, Geom G,
                                                              int zblk0 = 0, int byp0 = 0, int bx_0 = 0)
{
    __shared__ float t[kPcRows][PZ + 2];
    // (zblk0, byp0, bx_0): the first block of a sub-box conversion (diffus_convert_volume_box); 0 for a whole volume
    const int z0 = ((int)blockIdx.x + zblk0) * PZ;
    const int by0 = ((int)blockIdx.y + byp0) * 2, bx = blockIdx.z + bx_0;
    const int tid = threadIdx.x;
    for (int e = tid; e < kPcRows * (PZ + 1); e += kBlock) {
        int row = e / (PZ + 1), zz = e - row * (PZ + 1); // row = (x & 3) * 9 + column 0..8
        int x = min(bx * 4 + row / kPcCols, G.d0 - 1), y = min(by0 * 4 + row % kPcCols, G.d1 - 1), z = min(z0 + zz, G.d2 - 1);
        t[row][zz] = in[((long)x * G.d1 + y) * G.d2 + z];
    }
    __syncthreads();
    // float4 = the (z, z + 1) pairs of two neighbouring columns of one x-row: 10 per record
    constexpr int V4 = kPairFloats / 4;
    for (int e = tid; e < 2 * PZ * V4; e += kBlock) {
        const int half = e / (PZ * V4), r = e - half * (PZ * V4);
        const int zz = r / V4, q = r - zz * V4;       // q-th float4 of the record: pairs 2q and 2q + 1
        const int by = by0 + half;
        if (by < G.nb1 && z0 + zz < G.d2) {
            const int p0 = 2 * q, p1 = 2 * q + 1;     // pair index = (x & 3) * 5 + column
            const int r0 = (p0 / 5) * kPcCols + half * 4 + p0 % 5, r1 = (p1 / 5) * kPcCols + half * 4 + p1 % 5;
            const float4 v = make_float4(t[r0][zz], t[r0][zz + 1], t[r1][zz], t[r1][zz + 1]);
            const long rec = ((long)bx * G.nb1 + by) * G.d2 + z0 + zz;
            *reinterpret_cast<float4 *>(out + rec * kPairFloats + 4 * q) = v;
        }
    }
}

} // namespace

extern "C" {

size_t diffus_bricked_floats(int d0, int d1, int d2)
{
    if (d0 <= 0 || d1 <= 0 || d2 <= 0) return 0;
    return bricked_floats(d0, d1, d2);
}

size_t diffus_brick_count(int d0, int d1, int d2)
{
    if (d0 <= 0 || d1 <= 0 || d2 <= 0) return 0;
    return bricked_floats(d0, d1, d2) / kBrickFloats;
}

int diffus_gradbuf_flush(float *bricked, int *touched, int d0, int d1, int d2, float *vol, int accumulate,
                         diffus_stream_t stream)
{
    if (!bricked || !touched || !vol || d0 <= 0 || d1 <= 0 || d2 <= 0) return DIFFUS_EINVAL;
    if (accumulate < DIFFUS_FLUSH_STORE || accumulate > DIFFUS_FLUSH_DENSE) return DIFFUS_EINVAL;
    Geom G = make_geom(d0, d1, d2);
    const long nbricks = (long)(bricked_floats(d0, d1, d2) / kBrickFloats);
    if (reinterpret_cast<uintptr_t>(bricked) & 15) return DIFFUS_EINVAL; // a brick is read as 16-byte words
    const long per_wave = accumulate == DIFFUS_FLUSH_DENSE ? kWave : kFlushBricks;
    const long waves = (nbricks + per_wave - 1) / per_wave;
    const unsigned nblk = (unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
    if (accumulate == DIFFUS_FLUSH_DENSE)
        hipLaunchKernelGGL(gradbuf_flush_dense_kernel, dim3(nblk), dim3(kBlock), 0, (hipStream_t)stream, bricked, touched, vol,
                           G, nbricks);
    else if (!(d2 & 1) && !(reinterpret_cast<uintptr_t>(vol) & 7))
        hipLaunchKernelGGL(gradbuf_flush_kernel<true>, dim3(nblk), dim3(kBlock), 0, (hipStream_t)stream, bricked, touched, vol,
                           G, nbricks, accumulate);
    else
        hipLaunchKernelGGL(gradbuf_flush_kernel<false>, dim3(nblk), dim3(kBlock), 0, (hipStream_t)stream, bricked, touched, vol,
                           G, nbricks, accumulate);
    return last_launch();
}

size_t diffus_paired_floats(int d0, int d1, int d2)
{
    if (d0 <= 0 || d1 <= 0 || d2 <= 0) return 0;
    return paired_floats(d0, d1, d2);
}

int diffus_pair_volume(const float *vol, int d0, int d1, int d2, float *paired, diffus_stream_t stream)
{
    if (!vol || !paired || d0 <= 0 || d1 <= 0 || d2 <= 0) return DIFFUS_EINVAL;
    Geom G = make_geom(d0, d1, d2);
    dim3 grid((d2 + kPcZ - 1) / kPcZ, (G.nb1 + 1) / 2, (d0 + 3) / 4);
    if (grid.y > 65535 || grid.z > 65535) return DIFFUS_EUNSUPPORTED;
    hipLaunchKernelGGL(pair_convert_kernel<kPcZ>, grid, dim3(kBlock), 0, (hipStream_t)stream, vol, paired, G, 0, 0, 0);
    return last_launch();
}

int diffus_convert_volume_box(const float *vol, int d0, int d1, int d2, int layout, float *converted, int x0, int x1,
                              int y0, int y1, int z0, int z1, diffus_stream_t stream)
{
    if (!vol || !converted || d0 <= 0 || d1 <= 0 || d2 <= 0) return DIFFUS_EINVAL;
    if (layout != DIFFUS_BRICKED && layout != DIFFUS_PAIRED) return DIFFUS_EINVAL;
    if (x0 < 0 || y0 < 0 || z0 < 0 || x1 > d0 || y1 > d1 || z1 > d2) return DIFFUS_EINVAL;
    if (x0 >= x1 || y0 >= y1 || z0 >= z1) return DIFFUS_OK; // an empty box
    Geom G = make_geom(d0, d1, d2);
    const int bx_lo = x0 >> 2, bx_hi = (x1 - 1) >> 2; // brick rows (4 voxels of dim 0): no layout repeats a dim-0 neighbour
    // depths per block: the whole-volume kernels' (128 / 64: long coalesced rows) for a deep box, 8 for a thin one -- a
    // slice of constant dim 2, the plane every fan of the reference lies in, is two depths of records
    auto launch = [&](auto kernel_for, int per_block, int zlo, int zhi, int by_lo, int by_hi) { // depths zlo..zhi; by_lo..by_hi in blocks
        const dim3 grid(zhi / per_block - zlo / per_block + 1, by_hi - by_lo + 1, bx_hi - bx_lo + 1);
        if (grid.y > 65535 || grid.z > 65535) return (int)DIFFUS_EUNSUPPORTED;
        kernel_for(grid, zlo / per_block, by_lo);
        return last_launch();
    };
    hipStream_t st = (hipStream_t)stream;
    if (layout == DIFFUS_PAIRED) {
        // A record (brick column by, depth z) repeats the first column of brick column by + 1 and the depth z + 1: the
        // records that hold a voxel of [y0, y1) x [z0, z1) are brick columns (y0 - 1) / 4 .. (y1 - 1) / 4, depths z0 - 1 .. z1 - 1
        const int by_lo = max(y0 - 1, 0) >> 2, by_hi = (y1 - 1) >> 2, zr_lo = max(z0 - 1, 0), zr_hi = z1 - 1;
        if (zr_hi - zr_lo < 2 * kPcZThin)
            return launch([&](dim3 g, int zb, int byp) { hipLaunchKernelGGL(pair_convert_kernel<kPcZThin>, g, dim3(kBlock), 0, st, vol, converted, G, zb, byp, bx_lo); },
                          kPcZThin, zr_lo, zr_hi, by_lo >> 1, by_hi >> 1);
        return launch([&](dim3 g, int zb, int byp) { hipLaunchKernelGGL(pair_convert_kernel<kPcZ>, g, dim3(kBlock), 0, st, vol, converted, G, zb, byp, bx_lo); },
                      kPcZ, zr_lo, zr_hi, by_lo >> 1, by_hi >> 1);
    }
    const int by_lo = y0 >> 2, by_hi = (y1 - 1) >> 2;
    if (z1 - z0 <= 2 * kConvZThin)
        return launch([&](dim3 g, int zb, int by) { hipLaunchKernelGGL((brick_convert_kernel<true, false, kConvZThin>), g, dim3(kBlock), 0, st, vol, converted, G, zb, by, bx_lo); },
                      kConvZThin, z0, z1 - 1, by_lo, by_hi);
    return launch([&](dim3 g, int zb, int by) { hipLaunchKernelGGL((brick_convert_kernel<true, false, kConvZ>), g, dim3(kBlock), 0, st, vol, converted, G, zb, by, bx_lo); },
                  kConvZ, z0, z1 - 1, by_lo, by_hi);
}

int diffus_brick_volume(const float *vol, int d0, int d1, int d2, float *bricked, diffus_stream_t stream)
{
    if (!vol || !bricked || d0 <= 0 || d1 <= 0 || d2 <= 0) return DIFFUS_EINVAL;
    Geom G = make_geom(d0, d1, d2);
    dim3 grid((G.nb2 + kConvZ / 2 - 1) / (kConvZ / 2), G.nb1, (d0 + 3) / 4);
    if (grid.y > 65535 || grid.z > 65535) return DIFFUS_EUNSUPPORTED;
    hipLaunchKernelGGL((brick_convert_kernel<true, false>), grid, dim3(kBlock), 0, (hipStream_t)stream, vol, bricked, G, 0, 0, 0);
    return last_launch();
}

int diffus_unbrick_volume(const float *bricked, int d0, int d1, int d2, float *vol, int accumulate,
                          diffus_stream_t stream)
{
    if (!vol || !bricked || d0 <= 0 || d1 <= 0 || d2 <= 0) return DIFFUS_EINVAL;
    Geom G = make_geom(d0, d1, d2);
    dim3 grid((G.nb2 + kConvZ / 2 - 1) / (kConvZ / 2), G.nb1, (d0 + 3) / 4);
    if (grid.y > 65535 || grid.z > 65535) return DIFFUS_EUNSUPPORTED;
    if (accumulate)
        hipLaunchKernelGGL((brick_convert_kernel<false, true>), grid, dim3(kBlock), 0, (hipStream_t)stream, bricked, vol, G, 0, 0, 0);
    else
        hipLaunchKernelGGL((brick_convert_kernel<false, false>), grid, dim3(kBlock), 0, (hipStream_t)stream, bricked, vol, G, 0, 0, 0);
    return last_launch();
}

} // extern "C"
