// Stand-alone host check of the mesh clean-up entry points' argument handling (eslam_meshclean.hip): every call below is
// decided on the host, before any launch, so the program needs no GPU.  Built with the host side under AddressSanitizer and
// UndefinedBehaviorSanitizer by `make meshclean_host_check` and run on the CPU; exit status 0 = every expectation held.
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
    const int64_t LIM = ESLAM_MESH_MAX_COUNT;
    // workspace: 4 bytes a slot, slots = the power of two >= 2 V and >= ESLAM_MESH_WELD_MIN_SLOTS
    expect(eslam_mesh_weld_workspace_bytes(0) == 4 * ESLAM_MESH_WELD_MIN_SLOTS, "workspace, no vertices");
    expect(eslam_mesh_weld_workspace_bytes(1) == 4 * ESLAM_MESH_WELD_MIN_SLOTS, "workspace, one vertex");
    expect(eslam_mesh_weld_workspace_bytes(32) == 4 * 64, "workspace, 32 vertices");
    expect(eslam_mesh_weld_workspace_bytes(33) == 4 * 128, "workspace, 33 vertices");
    expect(eslam_mesh_weld_workspace_bytes(65) == 4 * 256, "workspace, 65 vertices");
    expect(eslam_mesh_weld_workspace_bytes(4096) == 4 * 8192, "workspace, a power of two");
    expect(eslam_mesh_weld_workspace_bytes(4097) == 4 * 16384, "workspace, one above a power of two");
    expect(eslam_mesh_weld_workspace_bytes(LIM) == 4 * (2 * LIM), "workspace, the largest count");
    expect(eslam_mesh_weld_workspace_bytes(LIM + 1) == -1, "workspace, beyond the limit");
    expect(eslam_mesh_weld_workspace_bytes(-1) == -1, "workspace, negative");
    expect(strlen(eslam_last_error()) > 0, "an error message is left behind");
    // weld
    expect(eslam_mesh_weld(f, -1, bytes, idx, nullptr) != 0, "weld, negative vertices");
    expect(eslam_mesh_weld(f, LIM + 1, bytes, idx, nullptr) != 0, "weld, vertices beyond the limit");
    expect(eslam_mesh_weld(nullptr, 4, bytes, idx, nullptr) != 0, "weld, null vertices");
    expect(eslam_mesh_weld(f, 4, nullptr, idx, nullptr) != 0, "weld, null workspace");
    expect(eslam_mesh_weld(f, 4, bytes, nullptr, nullptr) != 0, "weld, null output");
    expect(eslam_mesh_weld(nullptr, 0, nullptr, nullptr, nullptr) == 0, "weld, no vertices is valid");
    // components
    expect(eslam_mesh_components(idx, -1, 4, idx + 32, nullptr) != 0, "components, negative faces");
    expect(eslam_mesh_components(idx, 1, -4, idx + 32, nullptr) != 0, "components, negative vertices");
    expect(eslam_mesh_components(idx, LIM + 1, 4, idx + 32, nullptr) != 0, "components, faces beyond the limit");
    expect(eslam_mesh_components(idx, 1, LIM + 1, idx + 32, nullptr) != 0, "components, vertices beyond the limit");
    expect(eslam_mesh_components(nullptr, 1, 4, idx + 32, nullptr) != 0, "components, null faces");
    expect(eslam_mesh_components(idx, 1, 4, nullptr, nullptr) != 0, "components, null labels");
    expect(eslam_mesh_components(idx, 1, 0, idx + 32, nullptr) != 0, "components, faces over no vertices");
    expect(eslam_mesh_components(nullptr, 0, 0, nullptr, nullptr) == 0, "components, an empty mesh is valid");
    // component sizes
    expect(eslam_mesh_component_sizes(idx, -1, idx + 16, 4, idx + 32, nullptr) != 0, "sizes, negative faces");
    expect(eslam_mesh_component_sizes(idx, 1, idx + 16, -4, idx + 32, nullptr) != 0, "sizes, negative vertices");
    expect(eslam_mesh_component_sizes(idx, LIM + 1, idx + 16, 4, idx + 32, nullptr) != 0, "sizes, faces beyond the limit");
    expect(eslam_mesh_component_sizes(idx, 1, idx + 16, LIM + 1, idx + 32, nullptr) != 0, "sizes, vertices beyond the limit");
    expect(eslam_mesh_component_sizes(nullptr, 1, idx + 16, 4, idx + 32, nullptr) != 0, "sizes, null faces");
    expect(eslam_mesh_component_sizes(idx, 1, nullptr, 4, idx + 32, nullptr) != 0, "sizes, null labels");
    expect(eslam_mesh_component_sizes(idx, 1, idx + 16, 4, nullptr, nullptr) != 0, "sizes, null counts");
    expect(eslam_mesh_component_sizes(idx, 1, idx + 16, 0, idx + 32, nullptr) != 0, "sizes, faces over no vertices");
    expect(eslam_mesh_component_sizes(nullptr, 0, nullptr, 0, nullptr, nullptr) == 0, "sizes, an empty mesh is valid");
    if (failures == 0) printf("meshclean host check ok\n");
    return failures ? 1 : 0;
}
