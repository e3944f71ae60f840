// so100_render.hip -- the two render kernels (gfx950) behind so100_render (include/so100_sim.h); the scene model and the trace are
// in so100_render.hpp.  Both kernels only READ the state matrix and run on the caller's stream.
//   so100_render_scene  : one lane per env: qpos -> the packed per-env scene record (camera frame, cube pose, capsules, pads).
//   so100_render_pixels : grid (ceil(H W / 1024), envs), 256 threads x 4 consecutive pixels; one env per workgroup, so the primitive
//                         loop is wave-uniform (its record is read through scalar loads) and only the hit bookkeeping diverges.
#include <hip/hip_runtime.h>
#include "so100_render.hpp"
#include "so100_task.hpp"

namespace so100 {

struct RenderCamArgs { float p[3], R[9]; };
struct RenderPixArgs { int W, H, HW; unsigned mask; float inv_f; int vec; };

__global__ __launch_bounds__(256) void so100_render_scene(const float* __restrict__ S, int n, int begin, int count, int end_cam, RenderCamArgs cam,
                                                          float* __restrict__ rec) {
    const int i = (int)(blockIdx.x*blockDim.x + threadIdx.x);
    if (i >= count) return;
    const int env = begin + i;
    float q[6], cp[3], cq[4];
#pragma unroll
    for (int j = 0; j < 6; j++) q[j] = S[(size_t)(SF_q0 + j)*n + env];
#pragma unroll
    for (int j = 0; j < 3; j++) cp[j] = S[(size_t)(SF_cube_x + j)*n + env];
#pragma unroll
    for (int j = 0; j < 4; j++) cq[j] = S[(size_t)(SF_cube_qw + j)*n + env];
    render_scene<float>(q, cp, cq, end_cam != 0, cam.p, cam.R, rec + (size_t)i*RS_STRIDE);
}
static_assert(SF_q1 == SF_q0 + 1 && SF_q5 == SF_q0 + 5 && SF_cube_z == SF_cube_x + 2 && SF_cube_qz == SF_cube_qw + 3, "qpos rows are contiguous");

template <int CAM>
__global__ __launch_bounds__(256) void so100_render_pixels(const float* __restrict__ scene, RenderPixArgs a, uint8_t* __restrict__ rgb,
                                                           float* __restrict__ depth, uint8_t* __restrict__ seg) {
    const int env = (int)blockIdx.y;
    const float* rec = scene + (size_t)env*RS_STRIDE;
    const int p0 = (int)(blockIdx.x*1024u + threadIdx.x*4u);
    if (p0 >= a.HW) return;
    int row = p0 / a.W, col = p0 - row*a.W;
    RenderPixel px[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (p0 + k < a.HW) {
            float dx, dy;
            pixel_ray<float>(CAM, a.W, a.H, a.inv_f, row, col, dx, dy);
            px[k] = render_trace<float>(rec, a.mask, dx, dy);
        } else {
            px[k] = RenderPixel{};
        }
        if (++col == a.W) { col = 0; row++; }
    }
    const size_t base = (size_t)env*(size_t)a.HW + (size_t)p0;
    if (a.vec && p0 + 4 <= a.HW) {       // H W % 4 == 0 and aligned buffers: every group of 4 pixels starts on a 4-byte (depth: 16-byte) boundary
        if (rgb) {
            uint32_t* d = reinterpret_cast<uint32_t*>(rgb + 3*base);
            d[0] = (uint32_t)px[0].rgb[0] | ((uint32_t)px[0].rgb[1] << 8) | ((uint32_t)px[0].rgb[2] << 16) | ((uint32_t)px[1].rgb[0] << 24);
            d[1] = (uint32_t)px[1].rgb[1] | ((uint32_t)px[1].rgb[2] << 8) | ((uint32_t)px[2].rgb[0] << 16) | ((uint32_t)px[2].rgb[1] << 24);
            d[2] = (uint32_t)px[2].rgb[2] | ((uint32_t)px[3].rgb[0] << 8) | ((uint32_t)px[3].rgb[1] << 16) | ((uint32_t)px[3].rgb[2] << 24);
        }
        if (depth) *reinterpret_cast<float4*>(depth + base) = make_float4(px[0].depth, px[1].depth, px[2].depth, px[3].depth);
        if (seg) *reinterpret_cast<uint32_t*>(seg + base) = (uint32_t)px[0].seg | ((uint32_t)px[1].seg << 8) | ((uint32_t)px[2].seg << 16) | ((uint32_t)px[3].seg << 24);
    } else {                              // the tail of a frame, or sizes / buffers without that alignment: byte (word) stores
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (p0 + k >= a.HW) break;
            if (rgb) { rgb[3*(base + k)] = px[k].rgb[0]; rgb[3*(base + k) + 1] = px[k].rgb[1]; rgb[3*(base + k) + 2] = px[k].rgb[2]; }
            if (depth) depth[base + k] = px[k].depth;
            if (seg) seg[base + k] = px[k].seg;
        }
    }
}

hipError_t render_launch(const float* state, const RenderLaunch& L, float* scene_buf, uint8_t* rgb, float* depth, uint8_t* seg, hipStream_t st) {
    RenderCamArgs cam;
    for (int i = 0; i < 3; i++) cam.p[i] = L.cam_p[i];
    for (int i = 0; i < 9; i++) cam.R[i] = L.cam_R[i];
    hipLaunchKernelGGL(so100_render_scene, dim3((unsigned)((L.count + 255)/256)), dim3(256), 0, st, state, L.n, L.begin, L.count,
                       L.camera == RCAM_END ? 1 : 0, cam, scene_buf);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    RenderPixArgs a;
    a.W = L.W; a.H = L.H; a.HW = L.W*L.H; a.mask = L.mask; a.inv_f = L.inv_f;
    a.vec = (a.HW % 4 == 0) && ((uintptr_t)rgb % 4 == 0) && ((uintptr_t)depth % 16 == 0) && ((uintptr_t)seg % 4 == 0);
    const unsigned gx = (unsigned)((a.HW + 1023)/1024);
    constexpr int MAXY = 65535;                             // grid.y limit: envs in chunks
    for (int c0 = 0; c0 < L.count; c0 += MAXY) {
        const int cn = L.count - c0 < MAXY ? L.count - c0 : MAXY;
        const size_t off = (size_t)c0*(size_t)a.HW;
        uint8_t* r = rgb ? rgb + 3*off : nullptr;
        float* d = depth ? depth + off : nullptr;
        uint8_t* s = seg ? seg + off : nullptr;
        if (L.camera == RCAM_END)
            hipLaunchKernelGGL(so100_render_pixels<RCAM_END>, dim3(gx, (unsigned)cn), dim3(256), 0, st, scene_buf + (size_t)c0*RS_STRIDE, a, r, d, s);
        else
            hipLaunchKernelGGL(so100_render_pixels<RCAM_SCENE>, dim3(gx, (unsigned)cn), dim3(256), 0, st, scene_buf + (size_t)c0*RS_STRIDE, a, r, d, s);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace so100
