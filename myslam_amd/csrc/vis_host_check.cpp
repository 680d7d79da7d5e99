// Stand-alone host check of the panel / metrics entry points' argument handling (eslam_vis.hip): every call below is
// decided on the host, before any launch, so the program needs no GPU.  Built with the host side under AddressSanitizer
// and UndefinedBehaviorSanitizer by `make vis_host_check` and run on the CPU; exit status 0 = every expectation held.
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
    alignas(16) static float img[64];
    alignas(16) static double d[8];
    alignas(16) static uint8_t bytes[1024];
    const int TH = ESLAM_SSIM_TILE_H, TW = ESLAM_SSIM_TILE_W;
    // workspace sizes: one double per tile and channel; four per reduction block
    expect(eslam_ssim_workspace_bytes(11, 11, 1) == 8, "ssim workspace, one output pixel");
    expect(eslam_ssim_workspace_bytes(TH + 10, TW + 10, 3) == 3 * 8, "ssim workspace, exactly one tile");
    expect(eslam_ssim_workspace_bytes(TH + 11, 2 * TW + 11, 3) == 2 * 3 * 3 * 8, "ssim workspace, one pixel past the tiles");
    expect(eslam_ssim_workspace_bytes(16384, 16384, 3) == (int64_t)((16374 + TH - 1) / TH) * ((16374 + TW - 1) / TW) * 3 * 8,
           "ssim workspace, largest image");
    expect(eslam_ssim_workspace_bytes(10, 11, 1) == -1, "ssim workspace, H below the window");
    expect(eslam_ssim_workspace_bytes(11, 11, 2) == -1, "ssim workspace, two channels");
    expect(eslam_frame_stats_workspace_bytes(1, 1) == 32, "stats workspace, one pixel");
    expect(eslam_frame_stats_workspace_bytes(64, ESLAM_STATS_BLOCK_PIXELS / 64) == 32, "stats workspace, one block exactly");
    expect(eslam_frame_stats_workspace_bytes(1, ESLAM_STATS_BLOCK_PIXELS + 1) == 64, "stats workspace, one pixel more");
    expect(eslam_frame_stats_workspace_bytes(16384, 16384) == ((int64_t)16384 * 16384 / ESLAM_STATS_BLOCK_PIXELS) * 32,
           "stats workspace, largest image");
    expect(eslam_frame_stats_workspace_bytes(0, 4) == -1 && eslam_frame_stats_workspace_bytes(4, 16385) == -1, "stats workspace, bad sizes");
    // eslam_ssim: everything that must come back before a launch (the pointers are never dereferenced on the host)
    expect(eslam_ssim(img, img + 16, 10, 64, 1, d, nullptr, d + 4, nullptr) != 0, "H below 11");
    expect(eslam_ssim(img, img + 16, 64, 10, 3, d, nullptr, d + 4, nullptr) != 0, "W below 11");
    expect(eslam_ssim(img, img + 16, -5, 64, 1, d, nullptr, d + 4, nullptr) != 0, "negative H");
    expect(eslam_ssim(img, img + 16, 16, 16385, 1, d, nullptr, d + 4, nullptr) != 0, "W too large");
    expect(eslam_ssim(img, img + 16, 16, 16, 2, d, nullptr, d + 4, nullptr) != 0, "two channels");
    expect(eslam_ssim(img, img + 16, 16, 16, 0, d, nullptr, d + 4, nullptr) != 0, "no channel");
    expect(eslam_ssim(nullptr, img + 16, 16, 16, 1, d, nullptr, d + 4, nullptr) != 0, "null image");
    expect(eslam_ssim(img, nullptr, 16, 16, 1, d, nullptr, d + 4, nullptr) != 0, "null second image");
    expect(eslam_ssim(img, img + 16, 16, 16, 1, nullptr, nullptr, d + 4, nullptr) != 0, "null workspace");
    expect(eslam_ssim(img, img + 16, 16, 16, 1, d, img + 32, nullptr, nullptr) != 0, "null mean");
    expect(strlen(eslam_last_error()) > 0, "an error message is left behind");
    // eslam_frame_stats
    expect(eslam_frame_stats(img, img, img, img, 0, 4, d, d + 4, nullptr) != 0, "empty image");
    expect(eslam_frame_stats(img, img, img, img, 4, 16385, d, d + 4, nullptr) != 0, "image too wide");
    expect(eslam_frame_stats(nullptr, img, img, img, 2, 2, d, d + 4, nullptr) != 0, "null depth");
    expect(eslam_frame_stats(img, img, img, nullptr, 2, 2, d, d + 4, nullptr) != 0, "null colour");
    expect(eslam_frame_stats(img, img, img, img, 2, 2, nullptr, d + 4, nullptr) != 0, "null stats workspace");
    expect(eslam_frame_stats(img, img, img, img, 2, 2, d, nullptr, nullptr) != 0, "null stats output");
    // eslam_vis_panel
    expect(eslam_vis_panel(img, img, img, img, 0, 2, d, bytes, bytes + 768, nullptr) != 0, "empty panel");
    expect(eslam_vis_panel(img, img, img, img, 2, 2, nullptr, bytes, bytes + 768, nullptr) != 0, "null stats");
    expect(eslam_vis_panel(img, img, img, img, 2, 2, d, nullptr, bytes + 768, nullptr) != 0, "null colour table");
    expect(eslam_vis_panel(img, img, img, img, 2, 2, d, bytes, nullptr, nullptr) != 0, "null panel");
    expect(eslam_vis_panel(img, nullptr, img, img, 2, 2, d, bytes, bytes + 768, nullptr) != 0, "null ground-truth depth");
    if (failures == 0) printf("vis host check ok\n");
    return failures ? 1 : 0;
}
