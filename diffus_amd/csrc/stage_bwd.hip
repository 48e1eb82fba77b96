// stage_bwd.hip -- backward of the stage-level functions `from src.renderer import *` hands to the notebooks, which the
// reference differentiates by composing them by hand (SURVEY.md D3, §8(c) caveat 2):
//   custom_nearest_sampler   reference src/renderer.py:741-759  (vals = Z[x,y,z], :758)  -> diffus_sample_points_bwd
//   trace_ray / simulate_rays                       :90-180, :35-71 (reflection :27-33) -> diffus_trace_rays_bwd
//   compute_gaussian_pulse                          :459-479 (F.conv1d, :477)           -> diffus_rows_conv1d_bwd
// The volume gradient is always CANONICAL (d0,d1,d2) float32, added into with no-return global_atomic_add_f32; what
// reads the volume (a nearest voxel or a trilinear cell) is the forward's own code (nearest_index, tri_sample, cell_at).
// Pose and pulse gradients are fixed-order sums: bitwise repeatable.
#include "diffus_host.hpp"

namespace {

// gz = d loss / d (value of a sample that read cell c) -> the canonical volume gradient: the voxel (nearest) or the 8
// corners with the forward's lerp weights (trilinear).  Shared by the point and the ray backward.
template <int SAMPLER>
__device__ __forceinline__ void scatter_cell(float *__restrict__ gvol, const Geom &G, const Cell &c, float gz)
{
    if (gz == 0.f) return;
    for_each_corner<SAMPLER>(c, gz, [&](int i, int j, int k, float v) {
        if (v != 0.f) atomicAdd(gvol + vox_off<DIFFUS_CANONICAL>(G, i, j, k), v);
    });
}

// g * d r / d Z1 and g * d r / d Z2 of r = (Z2 - Z1) / (Z1 + Z2) (reference src/renderer.py:33), with the operands torch's
// SubBackward, AddBackward and DivBackward use in float32: g / den to the numerator, -g * ((num / den) / den) to the
// denominator.  So a sample pair with Z1 + Z2 = 0 gives the inf / NaN autograd gives through compute_reflection_coeff.
__device__ __forceinline__ void reflect_grad(float z1, float z2, float g, float &g1, float &g2)
{
    const float den = z1 + z2;
    const float gn = __fdiv_rn(g, den), gd = -g * __fdiv_rn(reflect(z1, z2), den);
    g1 = gd - gn;
    g2 = gn + gd;
}

// custom_nearest_sampler backward at arbitrary points, one thread per point: gvalues -> gvol (nullable), and
// gpoints = gvalue * grad v(p) (trilinear; the border rule of tri_sample) or zeros (nearest).
template <int SAMPLER, int LAYOUT>
__global__ __launch_bounds__(kBlock) void sample_points_bwd_kernel(const float *__restrict__ vol, Geom G,
                                                                   const float *__restrict__ pts, long n,
                                                                   const float *__restrict__ gval, float *__restrict__ gvol,
                                                                   float *__restrict__ gpts)
{
    for (long t = (long)blockIdx.x * kBlock + threadIdx.x; t < n; t += (long)gridDim.x * kBlock) {
        const float p[3] = {pts[t * 3], pts[t * 3 + 1], pts[t * 3 + 2]};
        const float g = gval[t];
        if (gvol) scatter_cell<SAMPLER>(gvol, G, cell_at<SAMPLER>(G, p), g);
        if (gpts) {
            float q[3] = {0.f, 0.f, 0.f};
            if (SAMPLER == DIFFUS_TRILINEAR) {
                const TriSample s = tri_sample<LAYOUT, true>(vol, G, p[0], p[1], p[2]);
                q[0] = g * s.g0;
                q[1] = g * s.g1;
                q[2] = g * s.g2;
            }
            for (int c = 0; c < 3; ++c) gpts[t * 3 + c] = q[c];
        }
    }
}

// trace_rays backward, one wave per ray, the lanes over its samples in chunks of 64 (any S).  The impedances are sampled
// again rather than kept from the forward: the trilinear gradient has to gather the sample's 8 corners for grad v(p)
// anyway, which yields the value with them; the forward's `imp` may not even exist (simulate_rays asks for refl only);
// and keeping it would hold P*R*S floats between the two calls.  Neighbours Z_{k-1}, Z_{k+1} come from the adjacent lanes,
// across a chunk edge from the previous chunk's last lane and one extra sample of lane 63.
//   gz_k = gimp[k] + g * d r_{k-1} / d Z_k + g * d r_k / d Z_k   -> gvol (cell of sample k)
//   trilinear: gsrc_part[ray] = sum_k gz_k grad v(p_k),  gdirs[ray] = sum_k k gz_k grad v(p_k)  (wave sums, fixed order)
template <int SAMPLER, int LAYOUT, bool PR>
__global__ __launch_bounds__(kBlock) void trace_rays_bwd_kernel(Args A, const float *__restrict__ gimp,
                                                                const float *__restrict__ grefl, float *__restrict__ gvol,
                                                                float *__restrict__ gsrc_part, float *__restrict__ gdirs)
{
    const long w = (long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (w >= (long)A.P * A.R) return; // (wave-uniform)
    const int lane = threadIdx.x & 63, S = A.S;
    Pose ps;
    load_pose<PR ? 3 : 1>(ps, A.src, A.src_f64, A.dirs, A.dir_f64, w / A.R, w);
    float zlast = 0.f;                // Z of the previous chunk's last sample
    float gs[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f};
    for (int base = 0; base < S; base += kWave) {
        const int k = base + lane;
        const bool live = k < S;
        const int kk = live ? k : S - 1; // lanes past the end repeat the last sample; what they compute is dropped
        const float p[3] = {ray_point(ps, 0, kk), ray_point(ps, 1, kk), ray_point(ps, 2, kk)};
        float z;
        TriSample ts{};
        if (SAMPLER == DIFFUS_TRILINEAR) {
            ts = tri_sample<LAYOUT, true>(A.vol, A.G, p[0], p[1], p[2]);
            z = ts.v;
        } else {
            z = sample_value<SAMPLER, LAYOUT>(A.vol, A.G, p);
        }
        float znext = 0.f; // Z_{k+1} for lane 63: the next chunk's first sample
        if (grefl && lane == kWave - 1 && k + 1 < S) {
            const float pn[3] = {ray_point(ps, 0, k + 1), ray_point(ps, 1, k + 1), ray_point(ps, 2, k + 1)};
            znext = sample_value<SAMPLER, LAYOUT>(A.vol, A.G, pn);
        }
        const float zp = lane_prev(z, zlast), zn = lane_next(z, znext);
        zlast = lane_bcast(z, kWave - 1);
        float gz = 0.f;
        if (live) {
            if (gimp) gz = gimp[w * S + k];
            if (grefl) {
                float g1, g2;
                if (k >= 1) {
                    reflect_grad(zp, z, grefl[w * (S - 1) + k - 1], g1, g2);
                    gz += g2;
                }
                if (k + 1 < S) {
                    reflect_grad(z, zn, grefl[w * (S - 1) + k], g1, g2);
                    gz += g1;
                }
            }
            if (gvol) scatter_cell<SAMPLER>(gvol, A.G, cell_at<SAMPLER>(A.G, p), gz);
            if (SAMPLER == DIFFUS_TRILINEAR) {
                const float tg[3] = {gz * ts.g0, gz * ts.g1, gz * ts.g2};
                const float kf = (float)k;
                for (int c = 0; c < 3; ++c) {
                    gs[c] += tg[c];
                    gd[c] += kf * tg[c];
                }
            }
        }
    }
    if (SAMPLER == DIFFUS_TRILINEAR) {
        for (int c = 0; c < 3; ++c) {
            const float s = wave_sum_to_lane63(gs[c]), d = wave_sum_to_lane63(gd[c]);
            if (lane == kWave - 1) {
                if (gsrc_part) gsrc_part[w * 3 + c] = s;
                if (gdirs) gdirs[w * 3 + c] = d;
            }
        }
    }
}

// gsrc[pose] = the pose's per-ray partials summed in a fixed order (one block per pose)
__global__ __launch_bounds__(kBlock) void pose_sum_kernel(const float *__restrict__ part, int R, float *__restrict__ gsrc)
{
    __shared__ float sm[3 * kWavesPerBlock];
    const long pose = blockIdx.x;
    float a[3] = {0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < R; i += kBlock)
        for (int c = 0; c < 3; ++c) a[c] += part[(pose * R + i) * 3 + c];
    block_sums<3>(a, sm);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) gsrc[pose * 3 + c] = a[c];
}

// ---- rows_conv1d backward.  Forward: out[b][m] = sum_t k[t] * in[b][m + t - pad], m < M.
// gin[b][j] = sum_t k[t] * gout[b][j + pad - t]: the transposed correlation, grid-stride over (b, j).
__global__ __launch_bounds__(kBlock) void rows_conv1d_bwd_in_kernel(const float *__restrict__ k, const float *__restrict__ gout,
                                                                    float *__restrict__ gin, int B, int N, int L, int pad, int M)
{
    const long total = (long)B * N;
    for (long e = (long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long)gridDim.x * kBlock) {
        const int b = (int)(e / N), j = (int)(e - (long)b * N);
        float acc = 0.f;
        for (int t = 0; t < L; ++t) {
            const int m = j + pad - t;
            if (m >= 0 && m < M) acc = __builtin_fmaf(k[t], gout[(long)b * M + m], acc);
        }
        gin[e] = acc;
    }
}

constexpr int kConvTaps = 4; // taps per pass of the gkernel partials

// number of blocks of the gkernel partials: a function of the shape only, so that the sum order (and the result) does
// not depend on the device
unsigned conv_bwd_blocks(long total) { return (unsigned)std::min<long>((total + kBlock - 1) / kBlock, 256); }

// gkernel partials: block q sums gout[b][m] * in[b][m + t - pad] over its grid-stride share of (b, m), in float64, for
// every tap t -> part[q][t].  Fixed order throughout: thread-serial, then the DPP wave sum, then the waves in order.
__global__ __launch_bounds__(kBlock) void rows_conv1d_bwd_k_part_kernel(const float *__restrict__ in, const float *__restrict__ gout,
                                                                        double *__restrict__ part, int B, int N, int L, int pad,
                                                                        int M)
{
    __shared__ double sm[kConvTaps * kWavesPerBlock];
    const long total = (long)B * M;
    const int wib = threadIdx.x >> 6;
    for (int t0 = 0; t0 < L; t0 += kConvTaps) {
        double a[kConvTaps] = {};
        for (long e = (long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long)gridDim.x * kBlock) {
            const int b = (int)(e / M), m = (int)(e - (long)b * M);
            const double g = gout[e];
#pragma unroll
            for (int q = 0; q < kConvTaps; ++q) {
                const int j = m + t0 + q - pad;
                if (t0 + q < L && j >= 0 && j < N) a[q] += g * (double)in[(long)b * N + j];
            }
        }
#pragma unroll
        for (int q = 0; q < kConvTaps; ++q) {
            const double s = wave_sum_to_lane63(a[q]);
            if ((threadIdx.x & 63) == 63) sm[q * kWavesPerBlock + wib] = s;
        }
        __syncthreads();
        if (threadIdx.x < kConvTaps && t0 + (int)threadIdx.x < L) {
            double s = 0.0;
            for (int v = 0; v < kWavesPerBlock; ++v) s += sm[threadIdx.x * kWavesPerBlock + v];
            part[(long)blockIdx.x * L + t0 + threadIdx.x] = s;
        }
        __syncthreads(); // sm is written again by the next pass
    }
}

// gkernel[t] = sum over the blocks' partials, in block order
__global__ __launch_bounds__(kBlock) void rows_conv1d_bwd_k_sum_kernel(const double *__restrict__ part, int nblk, int L,
                                                                       float *__restrict__ gk)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= L) return;
    double s = 0.0;
    for (int q = 0; q < nblk; ++q) s += part[(long)q * L + t];
    gk[t] = (float)s;
}

long conv_out_len(int N, int L, int pad) { return (long)N + 2L * pad - L + 1; }

} // namespace

extern "C" {

int diffus_sample_points_bwd(const float *vol, int d0, int d1, int d2, int layout, const float *points, long n, int sampler,
                             const float *gvalues, float *gvol, float *gpoints, diffus_stream_t stream)
{
    if (!vol || !points || !gvalues || n <= 0 || d0 <= 0 || d1 <= 0 || d2 <= 0) return DIFFUS_EINVAL;
    if (sampler != DIFFUS_NEAREST && sampler != DIFFUS_TRILINEAR) return DIFFUS_EINVAL;
    if (layout != DIFFUS_CANONICAL && layout != DIFFUS_BRICKED && layout != DIFFUS_PAIRED) return DIFFUS_EINVAL;
    if (d0 > (1 << 24) || d1 > (1 << 24) || d2 > (1 << 24) || bricked_floats(d0, d1, d2) >= ((size_t)1 << 30)) return DIFFUS_EUNSUPPORTED;
    if (!gvol && !gpoints) return DIFFUS_OK;
    hipStream_t st = (hipStream_t)stream;
    if (sampler == DIFFUS_NEAREST && gpoints) { // rounding to an index passes nothing to the point
        if (hipMemsetAsync(gpoints, 0, sizeof(float) * 3 * (size_t)n, st) != hipSuccess) return DIFFUS_ELAUNCH;
        gpoints = nullptr;
        if (!gvol) return DIFFUS_OK;
    }
    const Geom G = make_geom(d0, d1, d2, layout);
    unsigned nb = (unsigned)((n + kBlock - 1) / kBlock);
    if (nb > 256u * 16u) nb = 256u * 16u;
    return dispatch_sl(sampler, layout, [&](auto S_, auto L_) {
        hipLaunchKernelGGL((sample_points_bwd_kernel<decltype(S_)::value, decltype(L_)::value>), dim3(nb), dim3(kBlock), 0, st,
                           vol, G, points, n, gvalues, gvol, gpoints);
        return last_launch();
    });
}

size_t diffus_trace_rays_bwd_workspace_bytes(int P, int R)
{
    if (P <= 0 || R <= 0) return 0;
    return align256(sizeof(float) * 3 * (size_t)P * R);
}

int diffus_trace_rays_bwd(const float *vol, int d0, int d1, int d2, int layout, const void *src, int src_dtype,
                          const void *dirs, int dirs_dtype, int P, int R, int S, int sampler, const float *gimp,
                          const float *grefl, float *gvol, float *gsrc, float *gdirs, void *workspace,
                          size_t workspace_bytes, diffus_stream_t stream)
{
    int rc = check_common(vol, d0, d1, d2, src, src_dtype, dirs, dirs_dtype, P, R, S, 0, sampler, layout, false);
    if (rc) return rc;
    const bool tri = sampler == DIFFUS_TRILINEAR;
    const bool per_ray = (src_dtype & DIFFUS_SRC_PER_RAY) != 0; // gsrc (P,R,3): the kernel's per-ray sums ARE the result
    if (tri && gsrc && !per_ray && (!workspace || workspace_bytes < diffus_trace_rays_bwd_workspace_bytes(P, R))) return DIFFUS_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const bool grad = gimp || (grefl && S > 1);
    // nearest (or no incoming gradient): no pose gradient -- zeros, as diffus_render_bwd writes
    if (gsrc && (!tri || !grad) && hipMemsetAsync(gsrc, 0, sizeof(float) * 3 * (size_t)P * (per_ray ? R : 1), st) != hipSuccess) return DIFFUS_ELAUNCH;
    if (gdirs && (!tri || !grad) && hipMemsetAsync(gdirs, 0, sizeof(float) * 3 * (size_t)P * R, st) != hipSuccess) return DIFFUS_ELAUNCH;
    if (!grad || !(gvol || (tri && (gsrc || gdirs)))) return DIFFUS_OK;
    const Workspace none{}; // the kernel reads the volume and the poses of Args only: no render workspace behind it
    Args A = make_args(vol, d0, d1, d2, layout, src, src_dtype, dirs, dirs_dtype, P, R, S, 0, 0.f, none);
    float *part = (tri && gsrc) ? (per_ray ? gsrc : (float *)workspace) : nullptr;
    const unsigned nblk = (unsigned)(((long)P * R + kWavesPerBlock - 1) / kWavesPerBlock);
    rc = dispatch_sl(sampler, layout, [&](auto S_, auto L_) {
        constexpr int SM = decltype(S_)::value, LY = decltype(L_)::value;
        if (per_ray)
            hipLaunchKernelGGL((trace_rays_bwd_kernel<SM, LY, true>), dim3(nblk), dim3(kBlock), 0, st,
                               A, gimp, (S > 1) ? grefl : nullptr, gvol, part, tri ? gdirs : nullptr);
        else
            hipLaunchKernelGGL((trace_rays_bwd_kernel<SM, LY, false>), dim3(nblk), dim3(kBlock), 0, st,
                               A, gimp, (S > 1) ? grefl : nullptr, gvol, part, tri ? gdirs : nullptr);
        return last_launch();
    });
    if (rc || !part || per_ray) return rc;
    hipLaunchKernelGGL(pose_sum_kernel, dim3((unsigned)P), dim3(kBlock), 0, st, part, R, gsrc);
    return last_launch();
}

size_t diffus_rows_conv1d_bwd_workspace_bytes(int B, int N, int L, int pad)
{
    if (B <= 0 || N <= 0 || L <= 0 || pad < 0) return 0;
    const long M = conv_out_len(N, L, pad);
    if (M <= 0 || M > 0x7fffffffL) return 0;
    return align256(sizeof(double) * (size_t)conv_bwd_blocks((long)B * M) * (size_t)L);
}

int diffus_rows_conv1d_bwd(const float *in, int B, int N, const float *kernel, int L, int pad, const float *gout, float *gin,
                           float *gkernel, void *workspace, size_t workspace_bytes, diffus_stream_t stream)
{
    if (!in || !kernel || !gout || B <= 0 || N <= 0 || L <= 0 || pad < 0) return DIFFUS_EINVAL;
    const long M = conv_out_len(N, L, pad);
    if (M <= 0 || M > 0x7fffffffL) return DIFFUS_EINVAL;
    if (gkernel && (!workspace || workspace_bytes < diffus_rows_conv1d_bwd_workspace_bytes(B, N, L, pad))) return DIFFUS_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (gin) {
        unsigned nb = (unsigned)(((long)B * N + kBlock - 1) / kBlock);
        if (nb > 4096u) nb = 4096u;
        hipLaunchKernelGGL(rows_conv1d_bwd_in_kernel, dim3(nb), dim3(kBlock), 0, st, kernel, gout, gin, B, N, L, pad, (int)M);
        int rc = last_launch();
        if (rc) return rc;
    }
    if (gkernel) {
        const unsigned nb = conv_bwd_blocks((long)B * M);
        double *part = (double *)workspace;
        hipLaunchKernelGGL(rows_conv1d_bwd_k_part_kernel, dim3(nb), dim3(kBlock), 0, st, in, gout, part, B, N, L, pad, (int)M);
        int rc = last_launch();
        if (rc) return rc;
        hipLaunchKernelGGL(rows_conv1d_bwd_k_sum_kernel, dim3((unsigned)((L + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, part,
                           (int)nb, L, gkernel);
        return last_launch();
    }
    return DIFFUS_OK;
}

} // extern "C"
