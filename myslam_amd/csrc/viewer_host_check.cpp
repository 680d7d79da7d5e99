// Stand-alone host check of the viewer entry points' argument handling (eslam_viewer.hip): every call below is decided on
// the host, before any launch, so the program needs no GPU.  Built with the host side under AddressSanitizer and
// UndefinedBehaviorSanitizer by `make viewer_host_check` and run on the CPU; exit status 0 = every expectation held.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/eslam_hip.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        fprintf(stderr, "FAILED: %s (last error: %s)\n", what, eslam_last_error());
        ++failures;
    }
}

int main() {
    alignas(16) static float f[64];
    alignas(16) static int32_t idx[16];
    alignas(16) static uint8_t bytes[1024];
    const float fx = 300.0f, cx = 7.5f, zn = 0.01f, zf = 20.0f;
    // workspace: 8 bytes a key, a 256-byte block of counters, 8 bytes a queue entry (12 faces x 1 tile; the cap of 2^19 entries)
    expect(eslam_viewer_workspace_bytes(0, 1, 16, 16) == 8 * 256 + 256 + 8, "workspace, no faces");
    expect(eslam_viewer_workspace_bytes(12, 2, 16, 16) == 2 * 8 * 256 + 256 + 2 * 12 * 8, "workspace, 12 faces, two views");
    expect(eslam_viewer_workspace_bytes(12, 0, 16, 16) == 0, "workspace, no views");
    expect(eslam_viewer_workspace_bytes(INT32_MAX, 3, 16384, 16384) ==
               (int64_t)3 * 8 * 16384 * 16384 + 256 + (int64_t)3 * 8 * (1 << 19), "workspace, largest sizes");
    expect(eslam_viewer_workspace_bytes(-1, 1, 16, 16) == -1, "workspace, negative faces");
    expect(eslam_viewer_workspace_bytes((int64_t)INT32_MAX + 1, 1, 16, 16) == -1, "workspace, faces beyond int32");
    expect(eslam_viewer_workspace_bytes(1, -1, 16, 16) == -1, "workspace, negative views");
    expect(eslam_viewer_workspace_bytes(1, 1, 0, 16) == -1 && eslam_viewer_workspace_bytes(1, 1, 16, 16385) == -1, "workspace, bad image");
    // begin
    expect(eslam_viewer_begin(1, 0, 16, bytes, nullptr) != 0, "begin, empty image");
    expect(eslam_viewer_begin(1, 16, 16385, bytes, nullptr) != 0, "begin, image too wide");
    expect(eslam_viewer_begin(-1, 16, 16, bytes, nullptr) != 0, "begin, negative views");
    expect(eslam_viewer_begin(1, 16, 16, nullptr, nullptr) != 0, "begin, null workspace");
    expect(strlen(eslam_last_error()) > 0, "an error message is left behind");
    expect(eslam_viewer_begin(0, 16, 16, nullptr, nullptr) == 0, "begin, no views is valid");
    // mesh
#define MESH(V, NV, F, NF, COL, W2C, VIEWS, FX, FY, H, W, ZN, ZF, WS) \
    eslam_viewer_mesh(V, NV, F, NF, COL, W2C, VIEWS, FX, FY, cx, cx, H, W, ZN, ZF, 1, 0, WS, nullptr)
    expect(MESH(f, 3, idx, 1, bytes, f, 1, fx, fx, 0, 16, zn, zf, bytes) != 0, "mesh, empty image");
    expect(MESH(f, 3, idx, 1, bytes, f, 1, fx, fx, 16385, 16, zn, zf, bytes) != 0, "mesh, image too tall");
    expect(MESH(f, -1, idx, 1, bytes, f, 1, fx, fx, 16, 16, zn, zf, bytes) != 0, "mesh, negative vertices");
    expect(MESH(f, (int64_t)INT32_MAX + 1, idx, 1, bytes, f, 1, fx, fx, 16, 16, zn, zf, bytes) != 0, "mesh, vertices beyond int32");
    expect(MESH(f, 3, idx, (int64_t)INT32_MAX + 1, bytes, f, 1, fx, fx, 16, 16, zn, zf, bytes) != 0, "mesh, faces beyond int32");
    expect(MESH(f, 3, idx, 1, bytes, f, -2, fx, fx, 16, 16, zn, zf, bytes) != 0, "mesh, negative views");
    expect(MESH(f, 3, idx, 1, bytes, f, 1, 0.0f, fx, 16, 16, zn, zf, bytes) != 0, "mesh, fx = 0");
    expect(MESH(f, 3, idx, 1, bytes, f, 1, fx, NAN, 16, 16, zn, zf, bytes) != 0, "mesh, fy not a number");
    expect(MESH(f, 3, idx, 1, bytes, f, 1, fx, fx, 16, 16, 0.0f, zf, bytes) != 0, "mesh, z_near = 0");
    expect(MESH(f, 3, idx, 1, bytes, f, 1, fx, fx, 16, 16, zn, INFINITY, bytes) != 0, "mesh, z_far infinite");
    expect(MESH(f, 3, idx, 1, bytes, f, 1, fx, fx, 16, 16, 2.0f, 1.0f, bytes) != 0, "mesh, z_far below z_near");
    expect(MESH(nullptr, 3, idx, 1, bytes, f, 1, fx, fx, 16, 16, zn, zf, bytes) != 0, "mesh, null vertices");
    expect(MESH(f, 3, nullptr, 1, bytes, f, 1, fx, fx, 16, 16, zn, zf, bytes) != 0, "mesh, null faces");
    expect(MESH(f, 3, idx, 1, bytes, nullptr, 1, fx, fx, 16, 16, zn, zf, bytes) != 0, "mesh, null poses");
    expect(MESH(f, 3, idx, 1, bytes, f, 1, fx, fx, 16, 16, zn, zf, nullptr) != 0, "mesh, null workspace");
    expect(MESH(f, 3, idx, 0, nullptr, f, 1, fx, fx, 16, 16, zn, zf, bytes) == 0, "mesh, no faces is valid");
    expect(MESH(f, 3, idx, 1, nullptr, f, 0, fx, fx, 16, 16, zn, zf, bytes) == 0, "mesh, no views is valid");
    // points
#define POINTS(P, N, COL, SIZE, W2C, VIEWS, FX, H, W, ZN, ZF, WS) \
    eslam_viewer_points(P, N, COL, 1, SIZE, W2C, VIEWS, FX, fx, cx, cx, H, W, ZN, ZF, WS, nullptr)
    expect(POINTS(f, 4, bytes, 0, f, 1, fx, 16, 16, zn, zf, bytes) != 0, "points, size 0");
    expect(POINTS(f, 4, bytes, ESLAM_VIEWER_MAX_POINT_SIZE + 1, f, 1, fx, 16, 16, zn, zf, bytes) != 0, "points, size too large");
    expect(POINTS(f, -4, bytes, 4, f, 1, fx, 16, 16, zn, zf, bytes) != 0, "points, negative count");
    expect(POINTS(f, 4, bytes, 4, f, 1, fx, 16, 0, zn, zf, bytes) != 0, "points, empty image");
    expect(POINTS(f, 4, bytes, 4, f, 1, INFINITY, 16, 16, zn, zf, bytes) != 0, "points, fx infinite");
    expect(POINTS(f, 4, bytes, 4, f, 1, fx, 16, 16, -1.0f, zf, bytes) != 0, "points, z_near negative");
    expect(POINTS(nullptr, 4, bytes, 4, f, 1, fx, 16, 16, zn, zf, bytes) != 0, "points, null points");
    expect(POINTS(f, 4, nullptr, 4, f, 1, fx, 16, 16, zn, zf, bytes) != 0, "points, null colours");
    expect(POINTS(f, 4, bytes, 4, nullptr, 1, fx, 16, 16, zn, zf, bytes) != 0, "points, null poses");
    expect(POINTS(f, 4, bytes, 4, f, 1, fx, 16, 16, zn, zf, nullptr) != 0, "points, null workspace");
    expect(POINTS(f, 0, nullptr, 4, f, 1, fx, 16, 16, zn, zf, bytes) == 0, "points, no points is valid");
    expect(POINTS(f, 4, bytes, 4, f, 0, fx, 16, 16, zn, zf, bytes) == 0, "points, no views is valid");
    // resolve
    expect(eslam_viewer_resolve(1, 0, 16, 255, 255, 255, bytes, bytes + 512, nullptr, nullptr) != 0, "resolve, empty image");
    expect(eslam_viewer_resolve(-1, 16, 16, 255, 255, 255, bytes, bytes + 512, nullptr, nullptr) != 0, "resolve, negative views");
    expect(eslam_viewer_resolve(1, 16, 16, 256, 255, 255, bytes, bytes + 512, nullptr, nullptr) != 0, "resolve, background above 255");
    expect(eslam_viewer_resolve(1, 16, 16, 255, -1, 255, bytes, bytes + 512, nullptr, nullptr) != 0, "resolve, background below 0");
    expect(eslam_viewer_resolve(1, 16, 16, 255, 255, 255, nullptr, bytes + 512, nullptr, nullptr) != 0, "resolve, null workspace");
    expect(eslam_viewer_resolve(1, 16, 16, 255, 255, 255, bytes, nullptr, nullptr, nullptr) != 0, "resolve, null image");
    expect(eslam_viewer_resolve(0, 16, 16, 255, 255, 255, nullptr, nullptr, nullptr, nullptr) == 0, "resolve, no views is valid");
    // vertex shading
    const float cam[3] = {0.0f, 0.0f, -1.0f}, cam_nan[3] = {0.0f, NAN, 0.0f};
    expect(eslam_shade_vertices(f, f + 16, bytes, -1, cam, 0.3f, bytes + 512, nullptr) != 0, "shade, negative vertices");
    expect(eslam_shade_vertices(f, f + 16, bytes, (int64_t)INT32_MAX + 1, cam, 0.3f, bytes + 512, nullptr) != 0, "shade, vertices beyond int32");
    expect(eslam_shade_vertices(f, f + 16, bytes, 4, cam, -0.1f, bytes + 512, nullptr) != 0, "shade, ambient below 0");
    expect(eslam_shade_vertices(f, f + 16, bytes, 4, cam, 1.5f, bytes + 512, nullptr) != 0, "shade, ambient above 1");
    expect(eslam_shade_vertices(f, f + 16, bytes, 4, cam, NAN, bytes + 512, nullptr) != 0, "shade, ambient not a number");
    expect(eslam_shade_vertices(f, f + 16, bytes, 4, nullptr, 0.3f, bytes + 512, nullptr) != 0, "shade, null camera centre");
    expect(eslam_shade_vertices(f, f + 16, bytes, 4, cam_nan, 0.3f, bytes + 512, nullptr) != 0, "shade, camera centre not finite");
    expect(eslam_shade_vertices(nullptr, f + 16, bytes, 4, cam, 0.3f, bytes + 512, nullptr) != 0, "shade, null vertices");
    expect(eslam_shade_vertices(f, nullptr, bytes, 4, cam, 0.3f, bytes + 512, nullptr) != 0, "shade, null normals");
    expect(eslam_shade_vertices(f, f + 16, bytes, 4, cam, 0.3f, nullptr, nullptr) != 0, "shade, null output");
    expect(eslam_shade_vertices(f, f + 16, bytes + 1, 4, cam, 0.3f, bytes + 512, nullptr) != 0, "shade, misaligned colours");
    expect(eslam_shade_vertices(f, f + 16, bytes, 4, cam, 0.3f, bytes + 513, nullptr) != 0, "shade, misaligned output");
    expect(eslam_shade_vertices(nullptr, nullptr, nullptr, 0, cam, 0.3f, nullptr, nullptr) == 0, "shade, no vertices is valid");
    if (failures == 0) printf("viewer host check ok\n");
    return failures ? 1 : 0;
}
