// Host instantiation (float) of the DEVICE render header, for CPU-side tests only: the same scene record and per-pixel trace as
// so100_render.hip, with so100_render's argument handling (default mask, free-camera pose and focal length in double).
// Not a product path: libso100sim.so never links this file.
#include "../../so100_mujoco_rl_amd/csrc/so100_render.hpp"
#include <cstddef>
using namespace so100;

extern "C" int rc_record_floats(void) { return RS_STRIDE; }

// qpos: [n][13] float (arm q0..q5, cube x y z, cube qw qx qy qz); free_cam: 7 floats or NULL; outputs [n][H][W](x3) or NULL.
// rec_out: [n][RS_STRIDE] scene records or NULL.
extern "C" int rc_render(const float* qpos, int n, int camera, int W, int H, unsigned mask, const float* free_cam,
                         unsigned char* rgb, float* depth, unsigned char* seg, float* rec_out) {
    if (mask == 0) mask = camera == RCAM_END ? RG_DEFAULT_END : RG_DEFAULT_SCENE;
    float cam_p[3] = { 0, 0, 0 }, cam_R[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    double fovy = RENDER_END_FOVY;
    if (camera == RCAM_SCENE) {
        double lookat[3] = { RENDER_SCENE_LOOKAT[0], RENDER_SCENE_LOOKAT[1], RENDER_SCENE_LOOKAT[2] };
        double dist = RENDER_SCENE_DISTANCE, az = RENDER_SCENE_AZIMUTH, el = RENDER_SCENE_ELEVATION;
        fovy = RENDER_SCENE_FOVY;
        if (free_cam) { lookat[0] = free_cam[0]; lookat[1] = free_cam[1]; lookat[2] = free_cam[2]; dist = free_cam[3]; az = free_cam[4]; el = free_cam[5]; fovy = free_cam[6]; }
        double p[3], R[9];
        free_camera_pose<double>(lookat, dist, az, el, p, R);
        for (int i = 0; i < 3; i++) cam_p[i] = (float)p[i];
        for (int i = 0; i < 9; i++) cam_R[i] = (float)R[i];
    }
    const float inv_f = (float)render_inv_focal(fovy, H);
    const size_t HW = (size_t)W*H;
    float rec[RS_STRIDE];
    for (int e = 0; e < n; e++) {
        const float* q = qpos + 13*(size_t)e;
        for (int i = 0; i < RS_STRIDE; i++) rec[i] = 0.0f;
        render_scene<float>(q, q + 6, q + 9, camera == RCAM_END, cam_p, cam_R, rec);
        if (rec_out) for (int i = 0; i < RS_STRIDE; i++) rec_out[(size_t)e*RS_STRIDE + i] = rec[i];
        for (int r = 0; r < H; r++)
            for (int c = 0; c < W; c++) {
                float dx, dy;
                pixel_ray<float>(camera, W, H, inv_f, r, c, dx, dy);
                const RenderPixel px = render_trace<float>(rec, mask, dx, dy);
                const size_t k = (size_t)e*HW + (size_t)r*W + c;
                if (rgb) { rgb[3*k] = px.rgb[0]; rgb[3*k + 1] = px.rgb[1]; rgb[3*k + 2] = px.rgb[2]; }
                if (depth) depth[k] = px.depth;
                if (seg) seg[k] = px.seg;
            }
    }
    return 0;
}
