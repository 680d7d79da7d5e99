// Stand-alone host check of the point-to-mesh distance entry points' argument handling (eslam_meshdist.hip): every call
// below is decided on the host, before any launch, so the program needs no GPU.  Built with the host side under
// AddressSanitizer and UndefinedBehaviorSanitizer by `make meshdist_host_check` and run on the CPU; exit status 0 = every
// expectation held.
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
    alignas(16) static int32_t idx[64];
    alignas(16) static uint8_t bytes[1024];
    alignas(16) static int64_t total[2];
    const float box[6] = {0.0f, 7.0f, 0.0f, 5.0f, 0.0f, 3.0f};          // a room: lo / hi per axis
    eslam_tri_grid_t g;
    // the plan: cells of two face extents, capped by ESLAM_TRI_MAX_CELLS
    expect(eslam_tri_grid_plan(1000, box, 0.5f, &g) == 0, "plan, a room");
    expect(g.dims[0] == 7 && g.dims[1] == 5 && g.dims[2] == 3 && g.entries == 0, "plan, 7 x 5 x 3 cells of 1 m");
    expect(g.cell > 1.0f && g.cell < 1.00001f, "plan, the edge is the float just above two extents");
    expect(eslam_tri_grid_plan(1000, box, 1e-4f, &g) == 0, "plan, tiny faces");
    expect((int64_t)g.dims[0] * g.dims[1] * g.dims[2] <= ESLAM_TRI_MAX_CELLS, "plan, tiny faces stay within the cell limit");
    expect(eslam_tri_grid_plan(1000, box, 0.0f, &g) == 0, "plan, no face extent");
    expect((int64_t)g.dims[0] * g.dims[1] * g.dims[2] <= 4 * 1000, "plan, no face extent: about a cell per face");
    expect(eslam_tri_grid_plan(1000, box, NAN, &g) == 0, "plan, NaN face extent falls back");
    const float flat[6] = {1.0f, 1.0f, 2.0f, 2.0f, 3.0f, 3.0f};
    expect(eslam_tri_grid_plan(4, flat, 0.0f, &g) == 0 && g.dims[0] * g.dims[1] * g.dims[2] == 1, "plan, one point: one cell");
    expect(eslam_tri_grid_plan(0, nullptr, 0.0f, &g) == 0 && g.dims[0] == 1 && g.entries == 0, "plan, no faces is valid");
    expect(eslam_tri_grid_plan(-1, box, 0.5f, &g) != 0, "plan, negative faces");
    expect(eslam_tri_grid_plan(4, nullptr, 0.5f, &g) != 0, "plan, null box");
    expect(eslam_tri_grid_plan(4, box, 0.5f, nullptr) != 0, "plan, null grid");
    const float bad[6] = {0.0f, NAN, 0.0f, 1.0f, 0.0f, 1.0f};
    expect(eslam_tri_grid_plan(4, bad, 0.5f, &g) != 0, "plan, NaN box");
    const float inverted[6] = {1.0f, 0.0f, 0.0f, 1.0f, 0.0f, 1.0f};
    expect(eslam_tri_grid_plan(4, inverted, 0.5f, &g) != 0, "plan, inverted box");
    expect(strlen(eslam_last_error()) > 0, "an error message is left behind");

    expect(eslam_tri_grid_plan(1000, box, 0.5f, &g) == 0, "plan again");
    // F = 0 and Q = 0 launch nothing
    expect(eslam_tri_workspace_bytes(&g) > 0, "workspace, no entries yet");
    expect(eslam_tri_build(nullptr, 0, nullptr, 0, &g, nullptr, nullptr) == 0, "build, no faces is valid");
    expect(eslam_tri_query(&g, nullptr, f, 4, INFINITY, 0, nullptr, f + 16, idx, nullptr, nullptr) == 0,
           "query, no entries: nothing to launch");
    g.entries = 12;
    expect(eslam_tri_query(&g, bytes, nullptr, 0, INFINITY, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0,
           "query, no queries is valid");
    expect(eslam_tri_query_workspace_bytes(&g, 0) > 0, "query workspace, no queries");
    // the entry count of a planned grid beyond int32: refused with the count in the text
    g.entries = ESLAM_TRI_MAX_ENTRIES;
    expect(eslam_tri_workspace_bytes(&g) > 48 * ESLAM_TRI_MAX_ENTRIES, "workspace, the largest entry count");
    g.entries = ESLAM_TRI_MAX_ENTRIES + 1;
    expect(eslam_tri_workspace_bytes(&g) == -1, "workspace, entries beyond int32");
    expect(strstr(eslam_last_error(), "2147483648") != nullptr, "workspace, the error names the count");
    expect(eslam_tri_build(f, 8, idx, 4, &g, bytes, nullptr) != 0, "build, entries beyond int32");
    expect(strstr(eslam_last_error(), "2147483648") != nullptr, "build, the error names the count");
    expect(eslam_tri_query(&g, bytes, f, 4, INFINITY, 0, bytes, f + 16, idx, nullptr, nullptr) != 0, "query, entries beyond int32");
    g.entries = -1;
    expect(eslam_tri_build(f, 8, idx, 4, &g, bytes, nullptr) != 0, "build, negative entries");
    g.entries = 12;
    // count
    expect(eslam_tri_count(f, -1, idx, 4, &g, total, nullptr) != 0, "count, negative vertices");
    expect(eslam_tri_count(f, 8, idx, -4, &g, total, nullptr) != 0, "count, negative faces");
    expect(eslam_tri_count(nullptr, 8, idx, 4, &g, total, nullptr) != 0, "count, null vertices");
    expect(eslam_tri_count(f, 8, nullptr, 4, &g, total, nullptr) != 0, "count, null faces");
    expect(eslam_tri_count(f, 0, idx, 4, &g, total, nullptr) != 0, "count, faces over no vertices");
    expect(eslam_tri_count(f, 8, idx, 4, &g, nullptr, nullptr) != 0, "count, null total");
    expect(eslam_tri_count(f, 8, idx, 4, nullptr, total, nullptr) != 0, "count, null grid");
    // build
    expect(eslam_tri_build(f, -1, idx, 4, &g, bytes, nullptr) != 0, "build, negative vertices");
    expect(eslam_tri_build(f, 8, idx, -4, &g, bytes, nullptr) != 0, "build, negative faces");
    expect(eslam_tri_build(nullptr, 8, idx, 4, &g, bytes, nullptr) != 0, "build, null vertices");
    expect(eslam_tri_build(f, 8, nullptr, 4, &g, bytes, nullptr) != 0, "build, null faces");
    expect(eslam_tri_build(f, 8, idx, 4, &g, nullptr, nullptr) != 0, "build, null workspace");
    expect(eslam_tri_build(f, 8, idx, 4, nullptr, bytes, nullptr) != 0, "build, null grid");
    // query
    expect(eslam_tri_query(nullptr, bytes, f, 4, INFINITY, 0, bytes, f + 16, idx, nullptr, nullptr) != 0, "query, null grid");
    expect(eslam_tri_query(&g, bytes, f, -4, INFINITY, 0, bytes, f + 16, idx, nullptr, nullptr) != 0, "query, negative queries");
    expect(eslam_tri_query(&g, bytes, f, 4, INFINITY, 2, bytes, f + 16, idx, nullptr, nullptr) != 0, "query, unknown flags");
    expect(eslam_tri_query(&g, bytes, f, 4, NAN, 0, bytes, f + 16, idx, nullptr, nullptr) != 0, "query, NaN max_dist");
    expect(eslam_tri_query(&g, nullptr, f, 4, INFINITY, 0, bytes, f + 16, idx, nullptr, nullptr) != 0, "query, null workspace");
    expect(eslam_tri_query(&g, bytes, nullptr, 4, INFINITY, 0, bytes, f + 16, idx, nullptr, nullptr) != 0, "query, null queries");
    expect(eslam_tri_query(&g, bytes, f, 4, INFINITY, 0, nullptr, f + 16, idx, nullptr, nullptr) != 0,
           "query, null query workspace in cell order");
    expect(eslam_tri_query(&g, bytes, f, 4, INFINITY, 0, bytes, nullptr, idx, nullptr, nullptr) != 0, "query, null dist");
    expect(eslam_tri_query(&g, bytes, f, 4, INFINITY, 0, bytes, f + 16, nullptr, nullptr, nullptr) != 0, "query, null face");
    expect(eslam_tri_query_workspace_bytes(&g, -1) == -1, "query workspace, negative queries");
    expect(eslam_tri_query_workspace_bytes(nullptr, 4) == -1, "query workspace, null grid");
    // an invalid grid
    eslam_tri_grid_t z = g;
    z.dims[1] = 0;
    expect(eslam_tri_workspace_bytes(&z) == -1, "workspace, a grid without cells");
    z = g;
    z.cell = 0.0f;
    expect(eslam_tri_build(f, 8, idx, 4, &z, bytes, nullptr) != 0, "build, a cell edge of 0");
    z = g;
    z.dims[0] = z.dims[1] = z.dims[2] = 1024;
    expect(eslam_tri_query(&z, bytes, f, 4, INFINITY, 0, bytes, f + 16, idx, nullptr, nullptr) != 0, "query, too many cells");
    if (failures == 0) printf("meshdist host check ok\n");
    return failures ? 1 : 0;
}
