// so100_render.hpp -- ray casting of the so100 scene (DESIGN.md "Rendering"): the per-env scene record built from qpos and the
// per-pixel trace.  Templated on the scalar T like the physics headers: float on the device (so100_render.hip), a host
// instantiation exists ONLY for the CPU tests (tests/_rendercheck; never linked into libso100sim.so).
//
// The render model, with the MJCF line behind every number ("scene:" = envs/model/env01.xml, "arm:" = envs/model/so_arm100_camera.xml,
// "ref:" = the reference's envs/ directory):
//   cameras   pinhole, square pixels, f = 0.5 H / tan(fovy / 2); camera frame x right, y up, looking along -z (MuJoCo).
//             end   : the wrist camera end_point_camera (arm:125, fovy 120), pose from task_poses(want_cam); ROW 0 IS THE BOTTOM of the
//                     view (the memory order of mjr_readPixels, which ref: env_base_02.py:81 flips before pasting it).  Ray of pixel
//                     (r, c): ((c + 0.5 - W/2)/f, (r + 0.5 - H/2)/f, -1).
//             scene : MuJoCo's free camera (ref: env_base_01.py:13-18), rows top-down like Gymnasium's rgb_array.  Ray of pixel (r, c):
//                     ((c + 0.5 - W/2)/f, (H/2 - r - 0.5)/f, -1).
//             A ray's depth parameter IS the camera-axis depth (its camera-frame z is -1).  Hits nearer than ZNEAR are dropped, hits at or
//             beyond ZFAR are sky.  A primitive is hit only where the ray ENTERS it (a camera inside a primitive does not see it).
//   geometry  floor (id 1), cube (2), arm stand-in capsules (3..7), finger pads (8..15); equal depths: the lower id wins.
//   shading   c = base (AMBIENT + HEAD_DIFFUSE max(0, n.(-fwd_cam)) + LIGHT_DIFFUSE max(0, n.l)) clamped to [0, 1], byte = (uint8)(255 c + 0.5);
//             sky (unlit) = SKY_TOP 0.5 (1 + d_z) for the unit world ray d.
#pragma once
#include "so100_physics.hpp"
#include "so100_cube.hpp"
#include "so100_contact.hpp"
#include <stdint.h>

namespace so100 {

// ---- the render model's constants --------------------------------------------------------------------
constexpr int RCAM_END = 0, RCAM_SCENE = 1;                                   // include/so100_sim.h: SO100_CAM_END / SO100_CAM_SCENE
constexpr unsigned RG_FLOOR = 1u, RG_CUBE = 2u, RG_LINKS = 4u, RG_PADS = 8u;   // geom_mask bits
constexpr unsigned RG_DEFAULT_END = RG_FLOOR | RG_CUBE;                       // what the reference's detector looks at (the arm's meshes are absent)
constexpr unsigned RG_DEFAULT_SCENE = RG_FLOOR | RG_CUBE | RG_LINKS;          // pads: collision group 3, hidden by MuJoCo's default view
constexpr int RENDER_END_W = 1080, RENDER_END_H = 1920;                       // ref: env_base_02.py:22-23
constexpr int RENDER_SCENE_W = 800, RENDER_SCENE_H = 800;                     // ref: env_base_01.py:48-49
constexpr double RENDER_END_FOVY = so100g::CAM_FOVY_DEG;                      // arm:125 fovy="120"
constexpr double RENDER_SCENE_FOVY = 45.0;                                    // MuJoCo's default visual/global fovy
constexpr double RENDER_SCENE_LOOKAT[3] = { 0.0, 0.0, 0.1 };                  // scene:9 <statistic center="0 0 0.1">
constexpr double RENDER_SCENE_DISTANCE = 1.25, RENDER_SCENE_AZIMUTH = 45.0, RENDER_SCENE_ELEVATION = -25.0;   // ref: env_base_01.py:13-18
constexpr double RENDER_EXTENT = 0.8;                                         // scene:9 <statistic extent="0.8">
constexpr float ZNEAR = float(0.01*RENDER_EXTENT);                            // MuJoCo's default visual/map znear 0.01 x extent
constexpr float ZFAR = float(50.0*RENDER_EXTENT);                             // MuJoCo's default visual/map zfar 50 x extent
constexpr float AMBIENT = 0.3f, HEAD_DIFFUSE = 0.6f;                          // scene:12 <headlight ambient="0.3" diffuse="0.6">
constexpr float LIGHT_DIFFUSE = 0.7f;                                         // MuJoCo's default light diffuse (scene:38 sets none)
// scene:38 <light dir="-0.5 -0.5 -1" directional="true">: l = normalize(0.5, 0.5, 1), the direction TOWARD the light
constexpr float LIGHT_L[3] = { float(0.5/1.2247448713915890), float(0.5/1.2247448713915890), float(1.0/1.2247448713915890) };
constexpr float SKY_TOP = 0.8f;                                               // scene:18 gradient skybox rgb1 0.8 (top) -> rgb2 0 (bottom)
constexpr float CHECKER = 0.1f;                                               // scene:19-21 texrepeat 5 per metre (texuniform), 2 x 2 checker
constexpr float CHECKER_A[3] = { 0.2f, 0.3f, 0.4f }, CHECKER_B[3] = { 0.1f, 0.2f, 0.3f };   // scene:19-20 rgb1 / rgb2
constexpr float CUBE_RGB[3] = { 0.0f, 1.0f, 0.0f };                           // scene:32 rgba="0 1 0 1"
constexpr float LINK_RGB[3] = { 1.0f, 0.331f, 0.0f };                         // arm:7 material "orange"
constexpr float PAD_RGB[3] = { 0.5f, 0.5f, 0.5f };                            // MuJoCo's default geom rgba
constexpr int SEG_SKY = 0, SEG_FLOOR = 1, SEG_CUBE = 2, SEG_LINK0 = 3, SEG_PAD0 = 8;

// ---- the per-env scene record (floats; everything the trace reads, world frame) ------------------------
// camera: position, rotation (row-major, column j = camera axis j); cube: centre, rotation; capsule k: end a, unit axis u, length,
// radius; pad g: centre; pad rotations: the two jaws' link rotations.  The pads' half sizes are compile-time constants.
enum : int { RS_CAM_P = 0, RS_CAM_R = 3, RS_CUBE_P = 12, RS_CUBE_R = 15, RS_CAP = 24, RS_CAP_STRIDE = 8, RS_PAD_C = RS_CAP + 5*RS_CAP_STRIDE,
             RS_PAD_R4 = RS_PAD_C + 24, RS_PAD_R5 = RS_PAD_R4 + 9, RS_USED = RS_PAD_R5 + 9, RS_STRIDE = 112 };
static_assert(RS_USED <= RS_STRIDE && RS_STRIDE % 4 == 0, "scene record layout");
static_assert(so100g::NPROX == 5 && so100g::NPAD == 8, "render geometry counts");

// MuJoCo's free camera (mjv_cameraFrame): forward (cos e cos a, cos e sin a, sin e), up (-sin e cos a, -sin e sin a, cos e),
// position lookat - distance forward; camera axes x = forward x up, y = up, z = -forward.  Angles in degrees.
template <typename T> SO100_HD void free_camera_pose(const T lookat[3], T distance, T azimuth_deg, T elevation_deg, T pos[3], T R[9]) {
    const T deg = T(3.14159265358979323846/180.0);
    T sa, ca, se, ce;
    tsincos<T>(azimuth_deg*deg, sa, ca); tsincos<T>(elevation_deg*deg, se, ce);
    const T fwd[3] = { ce*ca, ce*sa, se }, up[3] = { -se*ca, -se*sa, ce };
    T right[3]; cross(fwd, up, right);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        pos[i] = lookat[i] - distance*fwd[i];
        R[3*i + 0] = right[i]; R[3*i + 1] = up[i]; R[3*i + 2] = -fwd[i];
    }
}

// the scene record of one env from its qpos (q: arm joints, cp / cq: cube position / quaternion w x y z).  end_cam: the camera
// is the wrist camera (task_poses); otherwise cam_p / cam_R (the free camera, the same for every env) are copied in.
template <typename T> SO100_HD void render_scene(const T q[6], const T cp[3], const T cq[4], bool end_cam, const T cam_p[3], const T cam_R[9], T* rec) {
    T s[6], c[6];
#pragma unroll
    for (int i = 0; i < 6; i++) tsincos<T>(q[i], s[i], c[i]);
    if (end_cam) {
        TaskPoses<T> P; task_poses(s, c, true, P);
#pragma unroll
        for (int i = 0; i < 3; i++) rec[RS_CAM_P + i] = P.cam_pos[i];
#pragma unroll
        for (int i = 0; i < 9; i++) rec[RS_CAM_R + i] = P.cam_mat[i];
    } else {
#pragma unroll
        for (int i = 0; i < 3; i++) rec[RS_CAM_P + i] = cam_p[i];
#pragma unroll
        for (int i = 0; i < 9; i++) rec[RS_CAM_R + i] = cam_R[i];
    }
    T qn[4] = { cq[0], cq[1], cq[2], cq[3] }, Rc[9];
    quat_normalize(qn);                                    // mj_kinematics normalises free-joint quaternions
    quat_to_mat(qn, Rc);
#pragma unroll
    for (int i = 0; i < 3; i++) rec[RS_CUBE_P + i] = cp[i];
#pragma unroll
    for (int i = 0; i < 9; i++) rec[RS_CUBE_R + i] = Rc[i];
    WorldFK<T> W; world_fk(s, c, W);
    // capsule k on link l = k + 1 (so100g::PROX_*): from the link's joint origin to its child's (links 1-3) or to PROX_FAR (the jaws),
    // the same segments as the F_LINKS_FLOOR contact proxies (so100_contact.hpp)
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int l = k + 1;
        T a[3], b[3];
#pragma unroll
        for (int i = 0; i < 3; i++) a[i] = W.o[l][i];
        if (l <= 3) {
#pragma unroll
            for (int i = 0; i < 3; i++) b[i] = W.o[l + 1][i];
        } else {
            const T* R = l == 4 ? W.R4 : W.R5;
            const T f0 = T(so100g::PROX_FAR[k][0]), f1 = T(so100g::PROX_FAR[k][1]), f2 = T(so100g::PROX_FAR[k][2]);
#pragma unroll
            for (int i = 0; i < 3; i++) b[i] = a[i] + R[3*i]*f0 + R[3*i + 1]*f1 + R[3*i + 2]*f2;
        }
        const T u[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] };
        const T len = tsqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]);
        const T il = len > T(0) ? T(1)/len : T(0);
        T* cap = rec + RS_CAP + RS_CAP_STRIDE*k;
#pragma unroll
        for (int i = 0; i < 3; i++) { cap[i] = a[i]; cap[3 + i] = u[i]*il; }
        cap[6] = len; cap[7] = T(so100g::PROX_RADIUS[k]);
    }
#pragma unroll
    for (int g = 0; g < 8; g++) {
        const bool l5 = so100g::PAD_LINK[g] == 5;
        const T* R = l5 ? W.R5 : W.R4; const T* o = l5 ? W.o[5] : W.o[4];
        const T p0 = T(so100g::PAD_POS[g][0]), p1 = T(so100g::PAD_POS[g][1]), p2 = T(so100g::PAD_POS[g][2]);
#pragma unroll
        for (int i = 0; i < 3; i++) rec[RS_PAD_C + 3*g + i] = o[i] + R[3*i]*p0 + R[3*i + 1]*p1 + R[3*i + 2]*p2;
    }
#pragma unroll
    for (int i = 0; i < 9; i++) { rec[RS_PAD_R4 + i] = W.R4[i]; rec[RS_PAD_R5 + i] = W.R5[i]; }
}

// ---- ray / primitive tests.  The ray is o + t dn with dn a unit vector (t in metres); every test returns the ENTRY parameter or
// a value >= tbest (no hit / not nearer) and fills the normal only when it returns a nearer hit. -------------------------------------

// box with centre cen, rotation R (row-major, columns = box axes), half sizes h: slab test in the box frame, normal of the entry face
template <typename T> SO100_HD T ray_box(const T o[3], const T dn[3], const T* cen, const T* R, const T h[3], T tmin_, T tbest, T n[3]) {
    const T r0 = o[0] - cen[0], r1 = o[1] - cen[1], r2 = o[2] - cen[2];
    // bounding-sphere early-out: the circumsphere |h|
    const T tc = -(r0*dn[0] + r1*dn[1] + r2*dn[2]);
    const T l0 = r0 + tc*dn[0], l1 = r1 + tc*dn[1], l2 = r2 + tc*dn[2];
    const T hb2 = h[0]*h[0] + h[1]*h[1] + h[2]*h[2];
    if (l0*l0 + l1*l1 + l2*l2 > hb2) return tbest;
    T tn = T(-3.0e38), tf = T(3.0e38), sgn = T(0);
    int ax = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const T ob = R[k]*r0 + R[3 + k]*r1 + R[6 + k]*r2;        // column k . (o - cen)
        const T db = R[k]*dn[0] + R[3 + k]*dn[1] + R[6 + k]*dn[2];
        const T inv = T(1)/db;
        const T ta = (-h[k] - ob)*inv, tb = (h[k] - ob)*inv;
        const T lo = tmin(ta, tb), hi = tmax(ta, tb);
        if (lo > tn) { tn = lo; ax = k; sgn = db > T(0) ? T(-1) : T(1); }
        tf = tmin(tf, hi);
    }
    if (!(tn <= tf) || tn < tmin_ || !(tn < tbest)) return tbest;
    n[0] = sgn*R[ax]; n[1] = sgn*R[3 + ax]; n[2] = sgn*R[6 + ax];
    return tn;
}

// sphere entry (centre c, radius r); tbest if missed
template <typename T> SO100_HD T ray_sphere(const T o[3], const T dn[3], const T c[3], T r, T tbest) {
    const T r0 = o[0] - c[0], r1 = o[1] - c[1], r2 = o[2] - c[2];
    const T tc = -(r0*dn[0] + r1*dn[1] + r2*dn[2]);
    const T l0 = r0 + tc*dn[0], l1 = r1 + tc*dn[1], l2 = r2 + tc*dn[2];
    const T disc = r*r - (l0*l0 + l1*l1 + l2*l2);
    if (disc < T(0)) return tbest;
    const T t = tc - tsqrt(disc);
    return t < tbest ? t : tbest;
}

// capsule (end a, unit axis u, length len, radius r): the infinite cylinder clipped to the segment, plus the two end spheres.  The
// capsule is convex, so its entry is the nearest of the parts' entries; an entry nearer than tmin_ (camera inside / clipped) is no hit.
template <typename T> SO100_HD T ray_capsule(const T o[3], const T dn[3], const T* cap, T tmin_, T tbest, T n[3]) {
    const T a[3] = { cap[0], cap[1], cap[2] }, u[3] = { cap[3], cap[4], cap[5] };
    const T len = cap[6], r = cap[7];
    const T oc[3] = { o[0] - a[0], o[1] - a[1], o[2] - a[2] };
    {   // bounding sphere: midpoint, half length + radius
        const T h = T(0.5)*len;
        const T m0 = oc[0] - h*u[0], m1 = oc[1] - h*u[1], m2 = oc[2] - h*u[2];
        const T tc = -(m0*dn[0] + m1*dn[1] + m2*dn[2]);
        const T l0 = m0 + tc*dn[0], l1 = m1 + tc*dn[1], l2 = m2 + tc*dn[2];
        if (l0*l0 + l1*l1 + l2*l2 > (h + r)*(h + r)) return tbest;
    }
    const T BIG = T(3.0e38);
    T t = BIG;
    // cylinder: components perpendicular to u
    const T du = dn[0]*u[0] + dn[1]*u[1] + dn[2]*u[2], ou = oc[0]*u[0] + oc[1]*u[1] + oc[2]*u[2];
    const T dp[3] = { dn[0] - du*u[0], dn[1] - du*u[1], dn[2] - du*u[2] }, op[3] = { oc[0] - ou*u[0], oc[1] - ou*u[1], oc[2] - ou*u[2] };
    const T A = dp[0]*dp[0] + dp[1]*dp[1] + dp[2]*dp[2];
    if (A > T(1e-12)) {
        const T tc = -(op[0]*dp[0] + op[1]*dp[1] + op[2]*dp[2])/A;
        const T l0 = op[0] + tc*dp[0], l1 = op[1] + tc*dp[1], l2 = op[2] + tc*dp[2];
        const T disc = r*r - (l0*l0 + l1*l1 + l2*l2);
        if (disc >= T(0)) {
            const T tt = tc - tsqrt(disc/A);
            const T y = ou + tt*du;
            if (y >= T(0) && y <= len) t = tt;
        }
    }
    const T b[3] = { a[0] + len*u[0], a[1] + len*u[1], a[2] + len*u[2] };
    const T ta = ray_sphere(o, dn, a, r, BIG), tb = ray_sphere(o, dn, b, r, BIG);
    int part = 0;                                            // 0 cylinder, 1 sphere a, 2 sphere b
    if (ta < t) { t = ta; part = 1; }
    if (tb < t) { t = tb; part = 2; }
    if (!(t < BIG) || t < tmin_ || !(t < tbest)) return tbest;
    const T p[3] = { oc[0] + t*dn[0], oc[1] + t*dn[1], oc[2] + t*dn[2] };   // hit point relative to a
    const T y = part == 0 ? p[0]*u[0] + p[1]*u[1] + p[2]*u[2] : part == 1 ? T(0) : len;
    const T ir = T(1)/r;
#pragma unroll
    for (int i = 0; i < 3; i++) n[i] = (p[i] - y*u[i])*ir;
    return t;
}

struct RenderPixel { uint8_t rgb[3]; uint8_t seg; float depth; };

SO100_HD uint8_t shade_byte(float c) {
    c = c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);
    return (uint8_t)(255.0f*c + 0.5f);
}

// Trace the ray of camera-frame direction (dx, dy, -1) against the geometry selected by mask.
template <typename T> SO100_HD RenderPixel render_trace(const T* rec, unsigned mask, T dx, T dy) {
    const T o[3] = { rec[RS_CAM_P], rec[RS_CAM_P + 1], rec[RS_CAM_P + 2] };
    const T* Rc = rec + RS_CAM_R;
    T d[3];
#pragma unroll
    for (int i = 0; i < 3; i++) d[i] = Rc[3*i]*dx + Rc[3*i + 1]*dy - Rc[3*i + 2];
    const T dl = tsqrt(d[0]*d[0] + d[1]*d[1] + d[2]*d[2]);
    const T idl = T(1)/dl;
    const T dn[3] = { d[0]*idl, d[1]*idl, d[2]*idl };
    // depth s (camera axis) = t / |d|: compare in t
    const T tnear = T(ZNEAR)*dl;
    T tbest = T(ZFAR)*dl;
    int id = SEG_SKY;
    T n[3] = { T(0), T(0), T(1) };
    T base[3] = { T(0), T(0), T(0) };
    if ((mask & RG_FLOOR) && dn[2] < T(0)) {                 // plane z = 0, normal +z, seen from above only
        const T t = -o[2]/dn[2];
        if (t >= tnear && t < tbest) {
            tbest = t; id = SEG_FLOOR;
            const T x = o[0] + t*dn[0], y = o[1] + t*dn[1];
            const int ix = (int)tfloor(x/T(CHECKER)), iy = (int)tfloor(y/T(CHECKER));
            const bool even = ((ix + iy) & 1) == 0;
#pragma unroll
            for (int i = 0; i < 3; i++) base[i] = even ? T(CHECKER_A[i]) : T(CHECKER_B[i]);
        }
    }
    if (mask & RG_CUBE) {
        const T h[3] = { T(so100g::CUBE_HALF), T(so100g::CUBE_HALF), T(so100g::CUBE_HALF) };
        T nn[3];
        const T t = ray_box(o, dn, rec + RS_CUBE_P, rec + RS_CUBE_R, h, tnear, tbest, nn);
        if (t < tbest) {
            tbest = t; id = SEG_CUBE;
#pragma unroll
            for (int i = 0; i < 3; i++) { n[i] = nn[i]; base[i] = T(CUBE_RGB[i]); }
        }
    }
    if (mask & RG_LINKS) {
#pragma unroll 1
        for (int k = 0; k < 5; k++) {
            T nn[3];
            const T t = ray_capsule(o, dn, rec + RS_CAP + RS_CAP_STRIDE*k, tnear, tbest, nn);
            if (t < tbest) {
                tbest = t; id = SEG_LINK0 + k;
#pragma unroll
                for (int i = 0; i < 3; i++) { n[i] = nn[i]; base[i] = T(LINK_RGB[i]); }
            }
        }
    }
    if (mask & RG_PADS) {
#pragma unroll 1
        for (int g = 0; g < 8; g++) {
            const T h[3] = { T(so100g::PAD_SIZE[g][0]), T(so100g::PAD_SIZE[g][1]), T(so100g::PAD_SIZE[g][2]) };
            T nn[3];
            const T t = ray_box(o, dn, rec + RS_PAD_C + 3*g, rec + (g < 4 ? RS_PAD_R4 : RS_PAD_R5), h, tnear, tbest, nn);
            if (t < tbest) {
                tbest = t; id = SEG_PAD0 + g;
#pragma unroll
                for (int i = 0; i < 3; i++) { n[i] = nn[i]; base[i] = T(PAD_RGB[i]); }
            }
        }
    }
    static_assert(so100g::PAD_LINK[0] == 4 && so100g::PAD_LINK[3] == 4 && so100g::PAD_LINK[4] == 5 && so100g::PAD_LINK[7] == 5, "pads 0-3 on link 4");
    RenderPixel px;
    px.seg = (uint8_t)id;
    if (id == SEG_SKY) {
        const uint8_t v = shade_byte(float(T(SKY_TOP)*T(0.5)*(T(1) + dn[2])));
        px.rgb[0] = px.rgb[1] = px.rgb[2] = v;
        px.depth = ZFAR;
    } else {
        // headlight along the camera's viewing direction: -fwd_cam = camera z axis
        const T nz = n[0]*Rc[2] + n[1]*Rc[5] + n[2]*Rc[8];
        const T nl = n[0]*T(LIGHT_L[0]) + n[1]*T(LIGHT_L[1]) + n[2]*T(LIGHT_L[2]);
        const T k = T(AMBIENT) + T(HEAD_DIFFUSE)*tmax(nz, T(0)) + T(LIGHT_DIFFUSE)*tmax(nl, T(0));
#pragma unroll
        for (int i = 0; i < 3; i++) px.rgb[i] = shade_byte(float(base[i]*k));
        px.depth = float(tbest*idl);
    }
    return px;
}

// camera-frame ray of pixel (row, col): the end camera's rows run bottom-up, the scene camera's top-down
template <typename T> SO100_HD void pixel_ray(int camera, int W, int H, T inv_f, int row, int col, T& dx, T& dy) {
    dx = (T(col) + T(0.5) - T(0.5)*T(W))*inv_f;
    dy = camera == RCAM_END ? (T(row) + T(0.5) - T(0.5)*T(H))*inv_f : (T(0.5)*T(H) - T(row) - T(0.5))*inv_f;
}

// 1 / f for a vertical field of view (degrees) and an image height: f = 0.5 H / tan(fovy / 2); computed in double on the host
inline double render_inv_focal(double fovy_deg, int H) {
    double s, c;
    tsincos<double>(0.5*fovy_deg*(3.14159265358979323846/180.0), s, c);
    return (s/c)/(0.5*(double)H);
}

}  // namespace so100

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace so100 {
// one so100_render call, validated by the ABI layer (so100_sim.hip); the kernels are in so100_render.hip
struct RenderLaunch {
    int camera, W, H, begin, count, n;       // n: envs of the state matrix
    unsigned mask;                           // geometry bits (non-zero)
    float cam_p[3], cam_R[9];                // the scene camera's pose (ignored for the end camera)
    float inv_f;                             // 1 / focal length in pixels
};
hipError_t render_launch(const float* state, const RenderLaunch& L, float* scene_buf, uint8_t* rgb, float* depth, uint8_t* seg, hipStream_t st);
}  // namespace so100
#endif
