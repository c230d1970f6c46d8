// frame_ops.hip - image-level producers / consumers either side of render_rays:
//   k_ray_forms    : every ray batch the object-level and SSR front-ends hand to the renderer, one body over
//                    {source: pinhole pose | given rays | mesh vertex + normal} x {NDC off | on} x {output: [N, 11] batch | (o, d) alone}
//                      pose  -> [N, 11]   run_nerf_helpers.py:359-368 + run_nerf.py:99-128 | rays.py:27-67, 223-256
//                      (o,d) -> [N, 11]   run_nerf.py:106-128 (render(rays=...): every object-level training step)
//                      (v,n) -> [N, 11]   SSR/extract_colour_mesh.py:232-238 (one ray per mesh vertex, against its normal)
//                      NDC                run_nerf_helpers.py:381-399 (run_nerf.py:117-119: the LLFF configs)
//   k_frame_to_u8  : to8b of rendered maps on the device (run_nerf_helpers.py:13 | trainer.py:1242), so that an image
//                    loop (run_nerf.py:142-212 | trainer.py:1221-1389) moves a quarter of the bytes to the host
// Both are a few MB of traffic per frame - microseconds; they exist for EXACTNESS (one rounding order, the same bits
// on every device) and to take the small launches (~15 per pose, ~20 more for NDC, ~8 per given batch) and six host
// synchronisations out of the per-image loop.
//
// Rounding order of the ray generator.  The 2^9-frequency encoding turns a one-ulp difference of a direction into a
// 2e-4 phase error, so the reference's fp32 evaluation order is reproduced operation by operation.  What ATen does on the
// reference's CPU path was established against tests/golden/rays_generators.npz and at full frame sizes
// (800x800, 320x240; 1 and 8 threads):
//   dirs   x = (i - cx) / fx,  y = (j - cy) / fy      one fp32 subtraction, one true division
//   rays_d d_k = (x R[k][0] + y' R[k][1]) + z' R[k][2]  three products, two additions, left to right, NO fma - both for
//          torch.sum(dirs[..., None, :] * c2w[:3,:3], -1) (object-level) and for torch.matmul(R, dirs) (SSR)
//   |d|    = sqrt(fma(d2, d2, fma(d1, d1, d0 * d0)))   torch.norm's vectorised kernel contracts; then a true division
// NDC (ndc_rays as ATen evaluates it; against tests/golden/rays_generators.npz and uncurated_object_llff_ndc.npz), with the
// fp32 scalars sx = -1/(W/(2 focal)), sy = -1/(H/(2 focal)), nr = near plane, c2 = 2 nr, cm2 = -2 nr:
//   t    = (-(nr + o_z)) / d_z                         add, sign flip (-0 stays -0), true division
//   o'_k = o_k + (t d_k)                               product, then sum - no fma
//   rz   = 1 / o'_z                                    `scalar / tensor` is Tensor.__rtruediv__ = reciprocal() * scalar:
//   O    = ((sx o'_x) / o'_z, (sy o'_y) / o'_z, 1 + rz c2)       a correctly rounded reciprocal, THEN the product
//   D    = (sx (d_x / d_z - o'_x / o'_z), sy (d_y / d_z - o'_y / o'_z), rz cm2)   every quotient its own true division
// View directions are the world-space direction over its norm, taken before NDC.
// Vertex rays (extract_colour_mesh.py:232-238), with near and near_t as fp32 scalars - what ATen makes of a Python number next to a
// float tensor - and float64 vertices / normals rounded to nearest fp32 first (torch.FloatTensor(np.asarray(...)), :232, :235):
//   d = -n;   o_k = v_k - ((d_k near) near_t)            two products, each rounded, then the subtraction - no fma
//   columns 6, 7 = near, far;   view direction = d / |d| as above
// Built with -ffp-contract=off; every operation below is an explicit __f*_rn.  The vertex form and the eleven columns are also
// evaluated on the host (inerf_vertex_rays_host): rn_* below are the intrinsic on the device and the plain operator, fmaf and sqrtf
// (each correctly rounded, nothing contracted) on the host.
#include <hip/hip_runtime.h>

#include <math.h>

#include "layout.h"

namespace inerf {

int record(hipError_t e);

#define INERF_HD __host__ __device__ __forceinline__
#if defined(__HIP_DEVICE_COMPILE__)
INERF_HD float rn_mul(float a, float b) { return __fmul_rn(a, b); }
INERF_HD float rn_sub(float a, float b) { return __fsub_rn(a, b); }
INERF_HD float rn_div(float a, float b) { return __fdiv_rn(a, b); }
INERF_HD float rn_fma(float a, float b, float c) { return __fmaf_rn(a, b, c); }
#else
INERF_HD float rn_mul(float a, float b) { return a * b; }
INERF_HD float rn_sub(float a, float b) { return a - b; }
INERF_HD float rn_div(float a, float b) { return a / b; }
INERF_HD float rn_fma(float a, float b, float c) { return fmaf(a, b, c); }
#endif

enum { kSrcPose = 0, kSrcGiven = 1, kSrcVertex = 2 };

struct RayFormParams {
    const float* poses;        // [B] camera-to-world matrices, rows of 4 floats, `pose_stride` floats apart
    const float* static_poses; // optional: origin / direction come from these, view directions from `poses`
    const float* rays_o;       // given rays: rows of 3 floats, `o_stride` / `d_stride` floats apart
    const float* rays_d;
    long long o_stride, d_stride;
    float* out;                // [N, 11]; split output: origins [N, 3]
    float* out_d;              // split output: directions [N, 3]
    long long n_rays;          // B * H * W, or the number of given rays
    int pose_stride;
    int H, W;
    float fx, fy, cx, cy, near, far;
    int opengl;                // 1: dirs = (x, -y, -1) (object-level, SSR convention "opengl"); 0: (x, y, 1) ("opencv")
    float sx, sy, nr, c2, cm2; // NDC coefficients (see the header comment)
    const void* vertices;      // vertex form: rows of 3 floats (in_f64: doubles), `v_stride` / `n_stride` ELEMENTS apart
    const void* normals;
    long long v_stride, n_stride;
    int in_f64;
    float near_t;
};

__device__ __forceinline__ void rotate(const float* __restrict__ p, float x, float y, float z, float (&d)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
        d[k] = __fadd_rn(__fadd_rn(__fmul_rn(x, p[4 * k + 0]), __fmul_rn(y, p[4 * k + 1])), __fmul_rn(z, p[4 * k + 2]));
}

// ndc_rays (run_nerf_helpers.py:381-399), in place
__device__ __forceinline__ void ndc_project(const RayFormParams& p, float (&o)[3], float (&d)[3]) {
    const float t = __fdiv_rn(-__fadd_rn(p.nr, o[2]), d[2]);
    float q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = __fadd_rn(o[k], __fmul_rn(t, d[k]));
    const float rz = __fdiv_rn(1.0f, q[2]);            // a bare v_rcp_f32 is 1 ulp; this is the correctly rounded one
    o[0] = __fdiv_rn(__fmul_rn(p.sx, q[0]), q[2]);
    o[1] = __fdiv_rn(__fmul_rn(p.sy, q[1]), q[2]);
    o[2] = __fadd_rn(1.0f, __fmul_rn(rz, p.c2));
    const float dx = __fmul_rn(p.sx, __fsub_rn(__fdiv_rn(d[0], d[2]), __fdiv_rn(q[0], q[2])));
    const float dy = __fmul_rn(p.sy, __fsub_rn(__fdiv_rn(d[1], d[2]), __fdiv_rn(q[1], q[2])));
    d[0] = dx; d[1] = dy;
    d[2] = __fmul_rn(rz, p.cm2);
}

// extract_colour_mesh.py:232-235: the ray of one mesh vertex, cast against its normal from near * near_t in front of the surface
template <typename T>
INERF_HD void vertex_ray(const T* __restrict__ vtx, const T* __restrict__ nrm, float near, float near_t, float (&o)[3], float (&d)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = (float)vtx[k], n = (float)nrm[k];              // float64: round to nearest fp32, once
        d[k] = -n;
        o[k] = rn_sub(x, rn_mul(rn_mul(d[k], near), near_t));
    }
}

// the eleven floats of one ray: [o3, d3, near, far, v / |v|]
INERF_HD void ray_columns(const float (&o)[3], const float (&d)[3], const float (&v)[3], float near, float far, float* __restrict__ s) {
    // sqrtf, not __fsqrt_rn: the latter lowers to a bare v_sqrt_f32 (1 ulp); ocml's sqrtf carries the correctly-rounding fix-up
    const float nrm = sqrtf(rn_fma(v[2], v[2], rn_fma(v[1], v[1], rn_mul(v[0], v[0]))));
    s[0] = o[0]; s[1] = o[1]; s[2] = o[2];
    s[3] = d[0]; s[4] = d[1]; s[5] = d[2];
    s[6] = near; s[7] = far;
    s[8] = rn_div(v[0], nrm); s[9] = rn_div(v[1], nrm); s[10] = rn_div(v[2], nrm);
}

// SRC: rays from a pose, from rays_o / rays_d, or from a mesh vertex and its normal; NDC: ndc_project on origin and direction;
// SPLIT: write (o, d) as two [N, 3] tensors instead of the [N, 11] batch (no view direction, no near / far)
template <int SRC, bool NDC, bool SPLIT>
__global__ __launch_bounds__(256) void k_ray_forms(const RayFormParams p) {
    __shared__ float stage[256 * (SPLIT ? 6 : INERF_RAY_FLOATS)];
    const long long base = (long long)blockIdx.x * 256;
    const long long idx = base + threadIdx.x;
    if (idx < p.n_rays) {
        float o[3], d[3], v[3];
        if constexpr (SRC == kSrcGiven) {
            const float* __restrict__ ro = p.rays_o + idx * p.o_stride;
            const float* __restrict__ rd = p.rays_d + idx * p.d_stride;
#pragma unroll
            for (int k = 0; k < 3; ++k) { o[k] = ro[k]; d[k] = rd[k]; v[k] = d[k]; }
        } else if constexpr (SRC == kSrcVertex) {
            if (p.in_f64)
                vertex_ray(static_cast<const double*>(p.vertices) + idx * p.v_stride, static_cast<const double*>(p.normals) + idx * p.n_stride,
                           p.near, p.near_t, o, d);
            else
                vertex_ray(static_cast<const float*>(p.vertices) + idx * p.v_stride, static_cast<const float*>(p.normals) + idx * p.n_stride,
                           p.near, p.near_t, o, d);
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = d[k];
        } else {
            const long long hw = (long long)p.H * p.W;
            const int b = (int)(idx / hw);
            const int pix = (int)(idx - b * hw);
            const int j = pix / p.W, i = pix - j * p.W;
            const float x = __fdiv_rn(__fsub_rn((float)i, p.cx), p.fx);
            float y = __fdiv_rn(__fsub_rn((float)j, p.cy), p.fy);
            float z = 1.0f;
            if (p.opengl) { y = -y; z = -1.0f; }
            const float* __restrict__ cam = p.poses + (size_t)b * p.pose_stride;
            rotate(cam, x, y, z, v);                                   // view direction: always the moving camera's
            const float* __restrict__ src = cam;
            if (p.static_poses) {                                      // c2w_staticcam (run_nerf.py:103-105 | rays.py:240-243)
                src = p.static_poses + (size_t)b * p.pose_stride;
                rotate(src, x, y, z, d);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) d[k] = v[k];
            }
            o[0] = src[3]; o[1] = src[7]; o[2] = src[11];
        }
        if constexpr (NDC) ndc_project(p, o, d);                       // after v was taken: view directions stay world-space
        if constexpr (SPLIT) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { stage[threadIdx.x * 3 + k] = o[k]; stage[768 + threadIdx.x * 3 + k] = d[k]; }
        } else {
            ray_columns(o, d, v, p.near, p.far, stage + threadIdx.x * INERF_RAY_FLOATS);
        }
    }
    __syncthreads();
    // the block's 256 rays are 2816 (split: 2 x 768) consecutive floats of the output: write them coalesced
    const long long left = p.n_rays - base;
    const int n_block = (int)(left < 256 ? left : 256);
    if constexpr (SPLIT) {
        float* __restrict__ oo = p.out + base * 3;
        float* __restrict__ od = p.out_d + base * 3;
        for (int t = threadIdx.x; t < n_block * 3; t += 256) { oo[t] = stage[t]; od[t] = stage[768 + t]; }
    } else {
        float* __restrict__ out = p.out + base * INERF_RAY_FLOATS;
        for (int t = threadIdx.x; t < n_block * INERF_RAY_FLOATS; t += 256) out[t] = stage[t];
    }
}

static void set_ndc(RayFormParams& p, const inerf_ndc* ndc) {
    p.sx = p.sy = p.nr = p.c2 = p.cm2 = 0.0f;
    if (!ndc) return;
    p.sx = ndc->sx; p.sy = ndc->sy; p.nr = ndc->near_plane;
    p.c2 = 2.0f * ndc->near_plane;                     // exact: what fp32(2. * near) is
    p.cm2 = -2.0f * ndc->near_plane;
}

static RayFormParams given_params(const float* rays_o, long long o_stride, const float* rays_d, long long d_stride, long long n_rays) {
    RayFormParams p = {};
    p.rays_o = rays_o; p.rays_d = rays_d; p.o_stride = o_stride; p.d_stride = d_stride; p.n_rays = n_rays;
    return p;
}

// out[i] = (uint8)(255 * clip(in[i], 0, 1)) - numpy's float32 product, truncation toward zero.  NaN -> 0.
__global__ __launch_bounds__(256) void k_frame_to_u8(const float* __restrict__ in, unsigned char* __restrict__ out, long long n) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = in[i];
        const float c = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);          // NaN fails both comparisons and stays NaN
        out[i] = c == c ? (unsigned char)(int)__fmul_rn(255.0f, c) : (unsigned char)0;
    }
}

}  // namespace inerf

extern "C" int inerf_gen_rays_ndc(const float* poses, int pose_stride, const float* static_poses, int n_poses, int height, int width,
                                  float fx, float fy, float cx, float cy, float near, float far, uint32_t flags,
                                  const inerf_ndc* ndc, float* rays_out, void* stream) {
    using namespace inerf;
    if (n_poses == 0 || height == 0 || width == 0) return INERF_OK;
    if (!poses || !rays_out || n_poses < 0 || height < 0 || width < 0 || pose_stride < 12) return INERF_E_INVALID;
    RayFormParams p = {};
    p.poses = poses; p.static_poses = static_poses; p.out = rays_out;
    p.n_rays = (long long)n_poses * height * width;
    p.pose_stride = pose_stride; p.H = height; p.W = width;
    p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy; p.near = near; p.far = far;
    p.opengl = (flags & INERF_CAM_OPENGL) ? 1 : 0;
    set_ndc(p, ndc);
    const long long blocks = (p.n_rays + 255) / 256;
    if (blocks > 0x7fffffffLL) return INERF_E_UNSUPPORTED;
    if (ndc) hipLaunchKernelGGL((k_ray_forms<kSrcPose, true, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((k_ray_forms<kSrcPose, false, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    return record(hipGetLastError());
}

extern "C" int inerf_gen_rays(const float* poses, int pose_stride, const float* static_poses, int n_poses, int height, int width,
                              float fx, float fy, float cx, float cy, float near, float far, uint32_t flags, float* rays_out,
                              void* stream) {
    return inerf_gen_rays_ndc(poses, pose_stride, static_poses, n_poses, height, width, fx, fy, cx, cy, near, far, flags, nullptr,
                              rays_out, stream);
}

extern "C" int inerf_assemble_rays(const float* rays_o, int64_t o_stride, const float* rays_d, int64_t d_stride, int64_t n_rays,
                                   float near, float far, const inerf_ndc* ndc, float* rays_out, void* stream) {
    using namespace inerf;
    if (n_rays == 0) return INERF_OK;
    if (!rays_o || !rays_d || !rays_out || n_rays < 0 || o_stride < 3 || d_stride < 3) return INERF_E_INVALID;
    RayFormParams p = given_params(rays_o, o_stride, rays_d, d_stride, n_rays);
    p.out = rays_out; p.near = near; p.far = far;
    set_ndc(p, ndc);
    const long long blocks = (p.n_rays + 255) / 256;
    if (blocks > 0x7fffffffLL) return INERF_E_UNSUPPORTED;
    if (ndc) hipLaunchKernelGGL((k_ray_forms<kSrcGiven, true, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((k_ray_forms<kSrcGiven, false, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    return record(hipGetLastError());
}

extern "C" int inerf_ndc_rays(const float* rays_o, int64_t o_stride, const float* rays_d, int64_t d_stride, int64_t n_rays,
                              const inerf_ndc* ndc, float* o_out, float* d_out, void* stream) {
    using namespace inerf;
    if (n_rays == 0) return INERF_OK;
    if (!rays_o || !rays_d || !ndc || !o_out || !d_out || n_rays < 0 || o_stride < 3 || d_stride < 3) return INERF_E_INVALID;
    RayFormParams p = given_params(rays_o, o_stride, rays_d, d_stride, n_rays);
    p.out = o_out; p.out_d = d_out;
    set_ndc(p, ndc);
    const long long blocks = (p.n_rays + 255) / 256;
    if (blocks > 0x7fffffffLL) return INERF_E_UNSUPPORTED;
    hipLaunchKernelGGL((k_ray_forms<kSrcGiven, true, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    return record(hipGetLastError());
}

static bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// INERF_OK when the rows are ones both forms of inerf_vertex_rays take (n > 0)
static int vertex_args(const void* vertices, int64_t v_stride, const void* normals, int64_t n_stride, int64_t n, int in_dtype,
                       const float* rays_out) {
    if (in_dtype != INERF_DTYPE_F32 && in_dtype != INERF_DTYPE_F64) return INERF_E_INVALID;
    if (!vertices || !normals || !rays_out || n < 0 || v_stride < 3 || n_stride < 3) return INERF_E_INVALID;
    const uintptr_t a = in_dtype == INERF_DTYPE_F64 ? 8 : 4;
    if (misaligned(vertices, a) || misaligned(normals, a) || misaligned(rays_out, 4)) return INERF_E_INVALID;
    return INERF_OK;
}

extern "C" int inerf_vertex_rays(const void* vertices, int64_t v_stride, const void* normals, int64_t n_stride, int64_t n, int in_dtype,
                                 float near, float far, float near_t, float* rays_out, void* stream) {
    using namespace inerf;
    if (n == 0) return INERF_OK;
    const int rc = vertex_args(vertices, v_stride, normals, n_stride, n, in_dtype, rays_out);
    if (rc != INERF_OK) return rc;
    RayFormParams p = {};
    p.vertices = vertices; p.normals = normals; p.v_stride = v_stride; p.n_stride = n_stride;
    p.in_f64 = in_dtype == INERF_DTYPE_F64; p.near_t = near_t;
    p.n_rays = n; p.out = rays_out; p.near = near; p.far = far;
    const long long blocks = (p.n_rays + 255) / 256;
    if (blocks > 0x7fffffffLL) return INERF_E_UNSUPPORTED;
    hipLaunchKernelGGL((k_ray_forms<kSrcVertex, false, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    return record(hipGetLastError());
}

extern "C" int inerf_vertex_rays_host(const void* vertices, int64_t v_stride, const void* normals, int64_t n_stride, int64_t n,
                                      int in_dtype, float near, float far, float near_t, float* rays_out) {
    using namespace inerf;
    if (n == 0) return INERF_OK;
    const int rc = vertex_args(vertices, v_stride, normals, n_stride, n, in_dtype, rays_out);
    if (rc != INERF_OK) return rc;
    for (int64_t i = 0; i < n; ++i) {
        float o[3], d[3];
        if (in_dtype == INERF_DTYPE_F64)
            vertex_ray(static_cast<const double*>(vertices) + i * v_stride, static_cast<const double*>(normals) + i * n_stride, near, near_t, o, d);
        else
            vertex_ray(static_cast<const float*>(vertices) + i * v_stride, static_cast<const float*>(normals) + i * n_stride, near, near_t, o, d);
        ray_columns(o, d, d, near, far, rays_out + i * INERF_RAY_FLOATS);
    }
    return INERF_OK;
}

extern "C" int inerf_frame_to_u8(const float* values, int64_t n, unsigned char* out, void* stream) {
    using namespace inerf;
    if (n == 0) return INERF_OK;
    if (!values || !out || n < 0) return INERF_E_INVALID;
    long long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_frame_to_u8, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, values, out, (long long)n);
    return record(hipGetLastError());
}
