// Dense RGB-D odometry of the VO step: the role Open3D's rgbd_odometry_multi_scale (Hybrid, 20 / 10 / 5
// iterations) plays at BodySLAM_not_refactored/3DM/visual_odometry.py:97-120.  Open3D is un-vendored: parity unpinned; the algorithm
// is the statement in oracle/rgbd_odometry_ref.py (hybrid photometric + geometric Gauss-Newton on a 3-level pyramid, Huber losses),
// which these kernels implement term by term.  Two switches (the `flags` of bs_odo_accumulate / bs_odo_step): bit 0 = the target is
// read at the NEAREST pixel of the projected point (Open3D's association; default of the product) instead of bilinearly; bit 1 =
// Open3D's form of the robust step (J^T J unweighted, J^T applied to the Huber-clipped residual) instead of IRLS weights.
//
// All of it is HBM-bound streaming / reduction work on 1.2 MB images: images are fp32 in HBM (NaN = invalid depth), the per-pixel
// arithmetic runs in fp64 (the vector fp64 rate is not the limit), and one Gauss-Newton step is ONE kernel that reduces 29 sums
// (21 of the symmetric 6x6, 6 of the right-hand side, the cost, the inlier count) per block into a [blocks, 29] buffer plus a
// second, single-block kernel that adds the partials in a fixed order -- the result does not depend on scheduling.
#include "common.h"
#include "reduce.h"
#include "rigid3.h"

namespace bs {

constexpr int ODO_TERMS = 29;
constexpr int ODO_GRID = 256;     // blocks of a Gauss-Newton step (one per CU; each walks its pixels in a fixed order: deterministic partials)

// level 0 of a pyramid: depth in metres, <= 0 or > depth_max -> NaN; COLOR: and intensity = grey / 255 (the point-to-plane pyramids have none)
template <bool COLOR>
__global__ __launch_bounds__(256) void odo_prepare_kernel(const uint8_t* __restrict__ color, const float* __restrict__ depth, int64_t n, float depth_max,
                                                           float* __restrict__ inten, float* __restrict__ dout) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if constexpr (COLOR) {
        const double v = (0.299 * (double)color[3 * i] + 0.587 * (double)color[3 * i + 1] + 0.114 * (double)color[3 * i + 2]) / 255.0;
        inten[i] = (float)v;
    }
    const float d = depth[i];
    dout[i] = (d > 0.0f && d <= depth_max) ? d : __builtin_nanf("");
}

// pseudo-RGBD depth of the 3DM loop (3DM/slam_utils.py:212-220): z = u16 / depth_scale as fp32, z >= depth_trunc -> 0 (no measurement)
__global__ __launch_bounds__(256) void depth_u16_to_m_kernel(const uint16_t* __restrict__ d, int64_t n, float scale, float trunc, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float z = __fdiv_rn((float)d[i], scale);
    out[i] = z >= trunc ? 0.0f : z;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// level l -> l + 1: [1 4 6 4 1]^2 / 256 at every even pixel, replicate borders.  DEPTH: the weights run over the neighbours whose
// depth is within `thr` of the centre's (NaN neighbours drop out), NaN when the centre is invalid.
template <bool DEPTH>
__global__ __launch_bounds__(256) void odo_pyrdown_kernel(const float* __restrict__ src, int H, int W, float* __restrict__ dst, int h2, int w2, double thr) {
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= w2 || y >= h2) return;
    src += (int64_t)blockIdx.z * H * W;            // image blockIdx.z of a batch of contiguous [H, W] images
    dst += (int64_t)blockIdx.z * h2 * w2;
    const double k5[5] = {1.0 / 16, 4.0 / 16, 6.0 / 16, 4.0 / 16, 1.0 / 16};
    const double centre = (double)src[(int64_t)clampi(2 * y, 0, H - 1) * W + clampi(2 * x, 0, W - 1)];
    if (DEPTH && centre != centre) {
        dst[(int64_t)y * w2 + x] = __builtin_nanf("");
        return;
    }
    double s = 0.0, wsum = 0.0;
    for (int dy = 0; dy < 5; ++dy)
        for (int dx = 0; dx < 5; ++dx) {
            const double v = (double)src[(int64_t)clampi(2 * y + dy - 2, 0, H - 1) * W + clampi(2 * x + dx - 2, 0, W - 1)];
            const double w = k5[dy] * k5[dx];
            if (DEPTH) {
                if (fabs(v - centre) <= thr) {        // false for NaN
                    s += w * v;
                    wsum += w;
                }
            } else {
                s += w * v;
            }
        }
    dst[(int64_t)y * w2 + x] = (float)(DEPTH ? s / wsum : s);
}

// 3x3 Sobel / 8, replicate borders; NaN propagates
__global__ __launch_bounds__(256) void odo_sobel_kernel(const float* __restrict__ img, int H, int W, float* __restrict__ gx, float* __restrict__ gy) {
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= W || y >= H) return;
    img += (int64_t)blockIdx.z * H * W;
    gx += (int64_t)blockIdx.z * H * W;
    gy += (int64_t)blockIdx.z * H * W;
    auto at = [&](int yy, int xx) { return (double)img[(int64_t)clampi(yy, 0, H - 1) * W + clampi(xx, 0, W - 1)]; };
    const double a = at(y - 1, x - 1), b = at(y - 1, x), c = at(y - 1, x + 1), d = at(y, x - 1), f = at(y, x + 1), g = at(y + 1, x - 1), h = at(y + 1, x),
                 i = at(y + 1, x + 1);
    gx[(int64_t)y * W + x] = (float)(((c + 2.0 * f + i) - (a + 2.0 * d + g)) / 8.0);
    gy[(int64_t)y * W + x] = (float)(((g + 2.0 * h + i) - (a + 2.0 * b + c)) / 8.0);
}

struct OdoPose {
    double t[12];     // rows 0..2 of the source -> target 4x4
    double fx, fy, cx, cy;
};

// ---- what the two accumulate kernels (hybrid below, point-to-plane further down) share --------------------------------------------------
// Pair blockIdx.y of a batch: image y of every [batch, H, W] stack (the returned offset), its own partials, and its own pose when the
// pose lives on the device (the step entries chain steps without a host round trip)
__device__ __forceinline__ int64_t odo_pair(int H, int W, OdoPose& P, const double* __restrict__ T_dev, double* __restrict__& partial) {
    partial += (int64_t)blockIdx.y * gridDim.x * ODO_TERMS;
    if (T_dev) {
#pragma unroll
        for (int i = 0; i < 12; ++i) P.t[i] = T_dev[(int64_t)blockIdx.y * 12 + i];
    }
    return (int64_t)blockIdx.y * H * W;
}

// source pixel `pix` back-projected and moved to the target frame; false where its depth is invalid or it lands behind the camera
__device__ __forceinline__ bool odo_source_point(const float* __restrict__ Ds, int64_t pix, int W, const OdoPose& P, double& px, double& py, double& pz) {
    const int v = (int)(pix / W), u = (int)(pix % W);
    const double z = (double)Ds[pix];
    if (!(z == z)) return false;
    const double X = ((double)u - P.cx) * z / P.fx, Y = ((double)v - P.cy) * z / P.fy;
    px = P.t[0] * X + P.t[1] * Y + P.t[2] * z + P.t[3];
    py = P.t[4] * X + P.t[5] * Y + P.t[6] * z + P.t[7];
    pz = P.t[8] * X + P.t[9] * Y + P.t[10] * z + P.t[11];
    return pz > 0.0;
}

// Open3D's robust step: huber'(r) = r clipped to +-delta, and the Huber cost
__device__ __forceinline__ double huber_clip(double r, double delta) { return fabs(r) < delta ? r : copysign(delta, r); }
__device__ __forceinline__ double huber_cost(double r, double delta) { return fabs(r) < delta ? 0.5 * r * r : delta * (fabs(r) - 0.5 * delta); }

// one inlier's 29 terms onto a thread's totals: A(a, b) over the upper triangle in row-major order, g(a), the cost, the count
template <class FA, class FG>
__device__ __forceinline__ void odo_add_inlier(double (&tot)[ODO_TERMS], FA A, FG g, double cost) {
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) tot[k++] += A(a, b);
#pragma unroll
    for (int a = 0; a < 6; ++a) tot[21 + a] += g(a);
    tot[27] += cost;
    tot[28] += 1.0;
}

// The block tail: 29 per-thread totals become row blockIdx.x of `partial`.  Inside a wave the DOWN shuffle 32, 16, ..., 1 (lane 0 ends
// with the total), then the four waves as (w0 + w1) + (w2 + w3) -- not reduce.h's block_sum (xor butterfly, waves added in sequence): a
// different order of the same additions, so different last bits.
__device__ __forceinline__ void odo_block_tail(const double (&tot)[ODO_TERMS], double* __restrict__ partial) {
    __shared__ double red[4][ODO_TERMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < ODO_TERMS; ++k) {
        double s = tot[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < ODO_TERMS) partial[(int64_t)blockIdx.x * ODO_TERMS + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// one Gauss-Newton step's sums, per block.  FLAGS bit 0: nearest-pixel association; bit 1: Open3D's Huber form
template <int FLAGS>
__global__ __launch_bounds__(256) void odo_accumulate_kernel(const float* __restrict__ Is, const float* __restrict__ Ds, const float* __restrict__ It,
                                                              const float* __restrict__ Dt, const float* __restrict__ dIx, const float* __restrict__ dIy,
                                                              const float* __restrict__ dDx, const float* __restrict__ dDy, int H, int W, OdoPose P,
                                                              const double* __restrict__ T_dev, double outlier, double huber_d, double huber_i,
                                                              double* __restrict__ partial) {
    {
        const int64_t o = odo_pair(H, W, P, T_dev, partial);
        Is += o; Ds += o; It += o; Dt += o; dIx += o; dIy += o; dDx += o; dDy += o;
    }
    double tot[ODO_TERMS];
#pragma unroll
    for (int k = 0; k < ODO_TERMS; ++k) tot[k] = 0.0;
    for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < (int64_t)H * W; pix += (int64_t)gridDim.x * 256) {
        double px, py, pz;
        if (!odo_source_point(Ds, pix, W, P, px, py, pz)) continue;
        const double uf = P.fx * px / pz + P.cx, vf = P.fy * py / pz + P.cy;
        constexpr bool NEAREST = (FLAGS & 1) != 0;
        const double ur = round(uf), vr = round(vf);           // (round half away from zero, as roundf)
        if (!(NEAREST ? (ur >= 0.0 && ur <= (double)(W - 1) && vr >= 0.0 && vr <= (double)(H - 1))
                      : (uf >= 0.0 && uf <= (double)(W - 1) && vf >= 0.0 && vf <= (double)(H - 1))))
            continue;
        int u0 = (int)floor(uf), v0 = (int)floor(vf);
        u0 = u0 > W - 2 ? W - 2 : u0;
        v0 = v0 > H - 2 ? H - 2 : v0;
        u0 = u0 < 0 ? 0 : u0;
        v0 = v0 < 0 ? 0 : v0;
        const double au = uf - (double)u0, av = vf - (double)v0;
        const int64_t o00 = (int64_t)v0 * W + u0;
        const int64_t onn = (int64_t)(int)vr * W + (int)ur;
        auto bil = [&](const float* __restrict__ img) {
            if (NEAREST) return (double)img[onn];
            return (1.0 - av) * ((1.0 - au) * (double)img[o00] + au * (double)img[o00 + 1]) +
                   av * ((1.0 - au) * (double)img[o00 + W] + au * (double)img[o00 + W + 1]);
        };
        const double dt = bil(Dt), hx = bil(dDx), hy = bil(dDy);
        const double rD = dt - pz;
        if (!(dt == dt && hx == hx && hy == hy && fabs(rD) <= outlier)) continue;
        const double gx = bil(dIx), gy = bil(dIy);
        const double rI = bil(It) - (double)Is[pix];
        const double iz = 1.0 / pz;
        const double c0 = gx * P.fx * iz, c1 = gy * P.fy * iz, c2 = -(c0 * px + c1 * py) * iz;
        const double d0 = hx * P.fx * iz, d1 = hy * P.fy * iz, d2 = -(d0 * px + d1 * py) * iz;
        const double JI[6] = {-pz * c1 + py * c2, pz * c0 - px * c2, -py * c0 + px * c1, c0, c1, c2};
        const double JD[6] = {(-pz * d1 + py * d2) - py, (pz * d0 - px * d2) + px, -py * d0 + px * d1, d0, d1, d2 - 1.0};
        if constexpr ((FLAGS & 2) != 0) {
            // Open3D: sum J^T J unweighted, sum J^T huber'(r), cost = sum huber(r)
            const double qI = huber_clip(rI, huber_i), qD = huber_clip(rD, huber_d);
            odo_add_inlier(
                tot, [&](int a, int b) { return JI[a] * JI[b] + JD[a] * JD[b]; }, [&](int a) { return JI[a] * qI + JD[a] * qD; },
                huber_cost(rI, huber_i) + huber_cost(rD, huber_d));
        } else {
            const double wI = fabs(rI) <= huber_i ? 1.0 : huber_i / fabs(rI);
            const double wD = fabs(rD) <= huber_d ? 1.0 : huber_d / fabs(rD);
            odo_add_inlier(
                tot, [&](int a, int b) { return wI * JI[a] * JI[b] + wD * JD[a] * JD[b]; },
                [&](int a) { return wI * JI[a] * rI + wD * JD[a] * rD; }, wI * rI * rI + wD * rD * rD);
        }
    }
    odo_block_tail(tot, partial);
}

// delta = -(A + 1e-12 I)^-1 b by Gaussian elimination with partial pivoting, T <- exp(delta) T (left twist: omega = delta[0:3],
// nu = delta[3:6]); fewer than 6 inliers or a singular system leave T alone.  One thread: 6x6.
__device__ void odo_solve(const double* __restrict__ s29, double* __restrict__ T) {
    if (s29[28] < 6.0) return;
    double M[6][7];
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) {
            M[a][b] = s29[k];
            M[b][a] = s29[k];
            ++k;
        }
    for (int a = 0; a < 6; ++a) {
        M[a][a] += 1e-12;
        M[a][6] = -s29[21 + a];
    }
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        for (int r = c + 1; r < 6; ++r)
            if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
        if (!(fabs(M[piv][c]) > 0.0)) return;
        if (piv != c)
            for (int j = 0; j < 7; ++j) {
                const double t = M[c][j];
                M[c][j] = M[piv][j];
                M[piv][j] = t;
            }
        for (int r = c + 1; r < 6; ++r) {
            const double f = M[r][c] / M[c][c];
            for (int j = c; j < 7; ++j) M[r][j] -= f * M[c][j];
        }
    }
    double d[6];
    for (int r = 5; r >= 0; --r) {
        double v = M[r][6];
        for (int j = r + 1; j < 6; ++j) v -= M[r][j] * d[j];
        d[r] = v / M[r][r];
    }
    Rigid3 g;
    se3_exp(d, g);
    left_apply(g, T);
}

// The block partials of pair blockIdx.x added in a fixed order (wave w: terms w and w + 16, each lane-strided over the blocks) and, where
// T is given, the 6x6 solve + pose update in the same launch: a Gauss-Newton step is two dependent launches.  T == nullptr: the sums only.
__global__ __launch_bounds__(1024) void odo_finish_solve_kernel(const double* __restrict__ partial, int nblocks, double* __restrict__ out, double* __restrict__ T) {
    __shared__ double s29[ODO_TERMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    partial += (int64_t)blockIdx.x * nblocks * ODO_TERMS;      // pair blockIdx.x of a batch
    out += (int64_t)blockIdx.x * ODO_TERMS;
    for (int k = wave; k < ODO_TERMS; k += 16) {
        const double s = column_sum(partial, nblocks, ODO_TERMS, k, lane);
        if (lane == 0) {
            s29[k] = s;
            out[k] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && T) odo_solve(s29, T + (int64_t)blockIdx.x * 12);
}

// ---- frame-to-model tracking: point-to-plane against the ray-cast model depth ---------------------------------------------------------
// The role of Open3D's Model::TrackFrameToModel (point-to-plane, 6 / 3 / 1 iterations) behind the reference's MAP
// (BodySLAM_not_refactored/3DM/tsdf.py:56-107).  Open3D is un-vendored: parity unpinned; the algorithm is the statement in
// tests/_point_to_plane_ref.py.  The target of a level is ONE 16-byte record per pixel, (nx, ny, nz, z): the forward-difference
// normal of the depth map's vertices and the depth itself, so a source pixel's scattered nearest-pixel read is one aligned load
// (the hybrid step reads six maps there); the target vertex is rebuilt from (u, v, z).  The sums go through the same [blocks, 29]
// partials, the same pixel-to-block walk, block tail and finish / solve kernel as the hybrid step; level 0 is odo_prepare_kernel<false>.

// V(u, v) = ((u - cx) z / fx, (v - cy) z / fy, z); n = normalise((V(u+1, v) - V(u, v)) x (V(u, v+1) - V(u, v))), NaN on the last row
// and column, where one of the three depths is invalid, or where the cross product has zero length
__global__ __launch_bounds__(256) void odo_p2p_target_kernel(const float* __restrict__ depth, int H, int W, double fx, double fy, double cx, double cy,
                                                             float4* __restrict__ rec) {
    const int u = blockIdx.x * 16 + (threadIdx.x & 15), v = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (u >= W || v >= H) return;
    depth += (int64_t)blockIdx.z * H * W;
    rec += (int64_t)blockIdx.z * H * W;
    const int64_t o = (int64_t)v * W + u;
    const float zf = depth[o];
    const float nanf_ = __builtin_nanf("");
    float4 out = make_float4(nanf_, nanf_, nanf_, zf);
    if (u + 1 < W && v + 1 < H) {
        const double z = (double)zf, zr = (double)depth[o + 1], zd = (double)depth[o + W];
        if (z == z && zr == zr && zd == zd) {
            const double x0 = ((double)u - cx) * z / fx, y0 = ((double)v - cy) * z / fy;
            const double ax = ((double)(u + 1) - cx) * zr / fx - x0, ay = ((double)v - cy) * zr / fy - y0, az = zr - z;
            const double bx = ((double)u - cx) * zd / fx - x0, by = ((double)(v + 1) - cy) * zd / fy - y0, bz = zd - z;
            const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
            const double len = sqrt(nx * nx + ny * ny + nz * nz);
            if (len > 0.0) out = make_float4((float)(nx / len), (float)(ny / len), (float)(nz / len), zf);
        }
    }
    rec[o] = out;
}

// one point-to-plane Gauss-Newton step's sums, per block: A = sum J J^T unweighted, b = sum J clip(r, +-huber), cost = sum huber(r)
__global__ __launch_bounds__(256) void odo_p2p_accumulate_kernel(const float* __restrict__ Ds, const float4* __restrict__ rec, int H, int W, OdoPose P,
                                                                 const double* __restrict__ T_dev, double depth_diff, double huber,
                                                                 double* __restrict__ partial) {
    {
        const int64_t o = odo_pair(H, W, P, T_dev, partial);
        Ds += o; rec += o;
    }
    double tot[ODO_TERMS];
#pragma unroll
    for (int k = 0; k < ODO_TERMS; ++k) tot[k] = 0.0;
    for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < (int64_t)H * W; pix += (int64_t)gridDim.x * 256) {
        double px, py, pz;
        if (!odo_source_point(Ds, pix, W, P, px, py, pz)) continue;
        const double ur = round(P.fx * px / pz + P.cx), vr = round(P.fy * py / pz + P.cy);           // round half away from zero
        if (!(ur >= 0.0 && ur <= (double)(W - 1) && vr >= 0.0 && vr <= (double)(H - 1))) continue;    // (false for NaN: the index below is in range)
        const float4 t = rec[(int64_t)(int)vr * W + (int)ur];
        const double nx = (double)t.x, ny = (double)t.y, nz = (double)t.z, zt = (double)t.w;
        if (!(nx == nx && zt == zt)) continue;
        const double qx = (ur - P.cx) * zt / P.fx, qy = (vr - P.cy) * zt / P.fy;
        const double r = ((px - qx) * nx + (py - qy) * ny) + (pz - zt) * nz;
        if (!(fabs(r) <= depth_diff)) continue;
        const double J[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
        const double q = huber_clip(r, huber);
        odo_add_inlier(
            tot, [&](int a, int b) { return J[a] * J[b]; }, [&](int a) { return J[a] * q; }, huber_cost(r, huber));
    }
    odo_block_tail(tot, partial);
}

static int odo_grid(int H, int W) {
    const int64_t b = cdiv64((int64_t)H * W, 256);
    return (int)(b < ODO_GRID ? b : ODO_GRID);
}

}  // namespace bs

using namespace bs;
#define ODO_ENTRY(name) \
    if (!initialized()) { set_error("%s: call bs_init first", name); return BS_ERR_NOT_INIT; }

struct OdoMaps {       // the hybrid step's maps: source intensity and depth, target intensity, depth and their gradients
    const float *Is, *Ds, *It, *Dt, *dIx, *dIy, *dDx, *dDy;
};

// What the four Gauss-Newton entries share.  `iterations` times: the sums of `batch` pairs (the hybrid kernel of `flags` on the maps m, or
// with rec != nullptr the point-to-plane kernel on m.Ds and rec; gate = the residual's outlier bound), then the fixed-order reduction
// into out29.  T_dev: the poses live on the device and every reduction ends in the solve + pose update (the step entries); otherwise
// the sums are taken at the host pose T_host and nothing is solved (the accumulate entries: one pair, one iteration).
static int odo_run(const char* name, const OdoMaps& m, const float* rec, int flags, int batch, int H, int W, const double* K, const double* T_host,
                   double* T_dev, int iterations, double gate, double huber_d, double huber_i, double* partial, double* out29, void* stream) {
    ODO_ENTRY(name);
    BS_REQUIRE((rec ? m.Ds != nullptr : m.Is && m.Ds && m.It && m.Dt && m.dIx && m.dIy && m.dDx && m.dDy) && K && (T_host || T_dev) && partial && out29,
               "%s: null argument", name);
    BS_REQUIRE(H > 1 && W > 1 && iterations >= 0 && batch > 0 && batch <= 65535 && (reinterpret_cast<uintptr_t>(rec) & 15) == 0,
               "%s: bad geometry%s", name, rec ? " or unaligned target" : "");
    OdoPose P;
    for (int i = 0; i < 12; ++i) P.t[i] = T_dev ? 0.0 : T_host[i];
    P.fx = K[0]; P.fy = K[1]; P.cx = K[2]; P.cy = K[3];
    auto hybrid = odo_accumulate_kernel<0>;
    switch (flags & 3) {
        case 1: hybrid = odo_accumulate_kernel<1>; break;
        case 2: hybrid = odo_accumulate_kernel<2>; break;
        case 3: hybrid = odo_accumulate_kernel<3>; break;
    }
    const int nblocks = odo_grid(H, W);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    for (int it = 0; it < iterations; ++it) {
        if (rec)
            hipLaunchKernelGGL(odo_p2p_accumulate_kernel, dim3(nblocks, batch), dim3(256), 0, st, m.Ds, reinterpret_cast<const float4*>(rec), H, W, P,
                               (const double*)T_dev, gate, huber_d, partial);
        else
            hipLaunchKernelGGL(hybrid, dim3(nblocks, batch), dim3(256), 0, st, m.Is, m.Ds, m.It, m.Dt, m.dIx, m.dIy, m.dDx, m.dDy, H, W, P,
                               (const double*)T_dev, gate, huber_d, huber_i, partial);
        BS_CHECK_LAUNCH();
        hipLaunchKernelGGL(odo_finish_solve_kernel, dim3(batch), dim3(1024), 0, st, (const double*)partial, nblocks, out29, T_dev);
        BS_CHECK_LAUNCH();
    }
    return BS_OK;
}

extern "C" int bs_depth_u16_to_m(const uint16_t* depth_u16, int64_t n, double depth_scale, double depth_trunc, float* out, void* stream) {
    ODO_ENTRY("bs_depth_u16_to_m");
    BS_REQUIRE(n >= 0 && depth_scale > 0.0, "bs_depth_u16_to_m: bad argument");
    if (n == 0) return BS_OK;        // (an empty tensor's pointers are null: nothing to check)
    BS_REQUIRE(depth_u16 && out, "bs_depth_u16_to_m: null argument");
    hipLaunchKernelGGL(depth_u16_to_m_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), depth_u16, n,
                       (float)depth_scale, (float)depth_trunc, out);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_odo_prepare(const uint8_t* color, const float* depth, int32_t batch, int32_t H, int32_t W, double depth_max, float* intensity,
                              float* depth_out, void* stream) {
    ODO_ENTRY("bs_odo_prepare");
    BS_REQUIRE(color && depth && intensity && depth_out && H > 0 && W > 0 && batch > 0, "bs_odo_prepare: bad argument");
    const int64_t n = (int64_t)batch * H * W;
    hipLaunchKernelGGL(odo_prepare_kernel<true>, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), color, depth, n,
                       (float)depth_max, intensity, depth_out);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_odo_pyrdown(const float* src, int32_t batch, int32_t H, int32_t W, float* dst, int32_t is_depth, double depth_threshold,
                              void* stream) {
    ODO_ENTRY("bs_odo_pyrdown");
    BS_REQUIRE(src && dst && H > 1 && W > 1 && batch > 0 && batch <= 65535, "bs_odo_pyrdown: bad argument");
    const int h2 = (H + 1) / 2, w2 = (W + 1) / 2;
    const dim3 grid(cdiv(w2, 16), cdiv(h2, 16), batch);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (is_depth)
        hipLaunchKernelGGL(odo_pyrdown_kernel<true>, grid, dim3(256), 0, st, src, H, W, dst, h2, w2, depth_threshold);
    else
        hipLaunchKernelGGL(odo_pyrdown_kernel<false>, grid, dim3(256), 0, st, src, H, W, dst, h2, w2, 0.0);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_odo_sobel(const float* img, int32_t batch, int32_t H, int32_t W, float* gx, float* gy, void* stream) {
    ODO_ENTRY("bs_odo_sobel");
    BS_REQUIRE(img && gx && gy && H > 0 && W > 0 && batch > 0 && batch <= 65535, "bs_odo_sobel: bad argument");
    hipLaunchKernelGGL(odo_sobel_kernel, dim3(cdiv(W, 16), cdiv(H, 16), batch), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), img, H, W, gx, gy);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_odo_accumulate(const float* src_intensity, const float* src_depth, const float* tgt_intensity, const float* tgt_depth,
                                 const float* tgt_dIx, const float* tgt_dIy, const float* tgt_dDx, const float* tgt_dDy, int32_t H, int32_t W,
                                 const double* K, const double* T, double depth_outlier_trunc, double depth_huber, double intensity_huber,
                                 double* partial, double* out29, int32_t flags, void* stream) {
    return odo_run("bs_odo_accumulate", {src_intensity, src_depth, tgt_intensity, tgt_depth, tgt_dIx, tgt_dIy, tgt_dDx, tgt_dDy}, nullptr, flags, 1, H, W, K,
                   T, nullptr, 1, depth_outlier_trunc, depth_huber, intensity_huber, partial, out29, stream);
}

extern "C" int bs_odo_step(const float* src_intensity, const float* src_depth, const float* tgt_intensity, const float* tgt_depth,
                           const float* tgt_dIx, const float* tgt_dIy, const float* tgt_dDx, const float* tgt_dDy, int32_t batch, int32_t H, int32_t W,
                           const double* K, double* T_dev, int32_t iterations, double depth_outlier_trunc, double depth_huber,
                           double intensity_huber, double* partial, double* out29, int32_t flags, void* stream) {
    return odo_run("bs_odo_step", {src_intensity, src_depth, tgt_intensity, tgt_depth, tgt_dIx, tgt_dIy, tgt_dDx, tgt_dDy}, nullptr, flags, batch, H, W, K,
                   nullptr, T_dev, iterations, depth_outlier_trunc, depth_huber, intensity_huber, partial, out29, stream);
}

extern "C" int bs_odo_p2p_prepare(const float* depth, int32_t batch, int32_t H, int32_t W, double depth_max, float* depth_out, void* stream) {
    ODO_ENTRY("bs_odo_p2p_prepare");
    BS_REQUIRE(depth && depth_out && H > 0 && W > 0 && batch > 0, "bs_odo_p2p_prepare: bad argument");
    const int64_t n = (int64_t)batch * H * W;
    hipLaunchKernelGGL(odo_prepare_kernel<false>, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       (const uint8_t*)nullptr, depth, n, (float)depth_max, (float*)nullptr, depth_out);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_odo_p2p_target(const float* depth, int32_t batch, int32_t H, int32_t W, const double* K, float* target, void* stream) {
    ODO_ENTRY("bs_odo_p2p_target");
    BS_REQUIRE(depth && K && target && H > 1 && W > 1 && batch > 0 && batch <= 65535, "bs_odo_p2p_target: bad argument");
    BS_REQUIRE((reinterpret_cast<uintptr_t>(target) & 15) == 0, "bs_odo_p2p_target: target must be 16-byte aligned");
    hipLaunchKernelGGL(odo_p2p_target_kernel, dim3(cdiv(W, 16), cdiv(H, 16), batch), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), depth, H, W, K[0],
                       K[1], K[2], K[3], reinterpret_cast<float4*>(target));
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_odo_p2p_accumulate(const float* src_depth, const float* target, int32_t H, int32_t W, const double* K, const double* T,
                                     double depth_diff, double depth_huber, double* partial, double* out29, void* stream) {
    OdoMaps m{};
    m.Ds = src_depth;
    return odo_run("bs_odo_p2p_accumulate", m, target, 0, 1, H, W, K, T, nullptr, 1, depth_diff, depth_huber, 0.0, partial, out29, stream);
}

extern "C" int bs_odo_p2p_step(const float* src_depth, const float* target, int32_t batch, int32_t H, int32_t W, const double* K, double* T_dev,
                               int32_t iterations, double depth_diff, double depth_huber, double* partial, double* out29, void* stream) {
    OdoMaps m{};
    m.Ds = src_depth;
    return odo_run("bs_odo_p2p_step", m, target, 0, batch, H, W, K, nullptr, T_dev, iterations, depth_diff, depth_huber, 0.0, partial, out29, stream);
}
