// Stand-alone host check of the frame entry points' argument handling (eslam_frame.hip): every call below is decided on
// the host, before any launch, so the program needs no GPU.  Built with the host side under AddressSanitizer and
// UndefinedBehaviorSanitizer by `make host_check` and run on the CPU; exit status 0 = every expectation held.
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
    int H = -1, W = -1;
    // shapes: no stage, crop_size, crop_size + edge, colour larger than depth
    expect(eslam_frame_out_shape(680, 1200, 680, 1200, 0, 0, 0, &H, &W) == 0 && H == 680 && W == 1200, "replica shape");
    expect(eslam_frame_out_shape(480, 640, 480, 640, 384, 512, 8, &H, &W) == 0 && H == 368 && W == 496, "tum shape");
    expect(eslam_frame_out_shape(968, 1296, 480, 640, 0, 0, 10, &H, &W) == 0 && H == 460 && W == 620, "scannet shape");
    expect(eslam_frame_out_shape(16384, 16384, 16384, 16384, 16384, 16384, 8191, &H, &W) == 0 && H == 2 && W == 2, "largest sizes");
    // rejected geometry
    expect(eslam_frame_out_shape(0, 640, 480, 640, 0, 0, 0, &H, &W) != 0, "empty colour image");
    expect(eslam_frame_out_shape(480, 640, 480, 16385, 0, 0, 0, &H, &W) != 0, "depth image too wide");
    expect(eslam_frame_out_shape(480, 640, 480, 640, 384, 0, 0, &H, &W) != 0, "half a crop_size");
    expect(eslam_frame_out_shape(480, 640, 480, 640, -1, -1, 0, &H, &W) != 0, "negative crop_size");
    expect(eslam_frame_out_shape(480, 640, 480, 640, 0, 0, 240, &H, &W) != 0, "crop_edge eats the image");
    expect(eslam_frame_out_shape(480, 640, 480, 640, 0, 0, -1, &H, &W) != 0, "negative crop_edge");
    expect(eslam_frame_out_shape(480, 640, 480, 640, 0, 0, 2147483647, &H, &W) != 0, "crop_edge near INT_MAX");
    expect(eslam_frame_out_shape(480, 640, 480, 640, 0, 0, 0, nullptr, &W) != 0, "null output");
    expect(strlen(eslam_last_error()) > 0, "an error message is left behind");

    // eslam_frame_prepare: everything that must come back before a launch (the pointers are never dereferenced on the host)
    alignas(16) static uint8_t rgb[16];
    alignas(16) static uint16_t depth[16];
    alignas(16) static float out[64];
    expect(eslam_frame_prepare(rgb, 2, 2, depth, 2, 2, 0, 0, 1, 1000.0f, 1.0f, out, out + 16, nullptr) != 0, "edge eats a 2 x 2 image");
    expect(eslam_frame_prepare(rgb, 2, 2, depth, 2, 2, 0, 0, 0, 0.0f, 1.0f, out, out + 16, nullptr) != 0, "png_depth_scale 0");
    expect(eslam_frame_prepare(rgb, 2, 2, depth, 2, 2, 0, 0, 0, 1000.0f, __builtin_nanf(""), out, out + 16, nullptr) != 0, "scale NaN");
    expect(eslam_frame_prepare(nullptr, 2, 2, depth, 2, 2, 0, 0, 0, 1000.0f, 1.0f, out, out + 16, nullptr) != 0, "null colour");
    expect(eslam_frame_prepare(rgb, 2, 2, depth, 2, 2, 0, 0, 0, 1000.0f, 1.0f, out, nullptr, nullptr) != 0, "null depth output");
    expect(eslam_frame_prepare(rgb, 2, 2, (const uint16_t*)((const uint8_t*)depth + 1), 2, 2, 0, 0, 0, 1000.0f, 1.0f, out, out + 16, nullptr) != 0,
           "odd depth address");
    expect(eslam_frame_prepare(rgb, 2, 2, depth, 2, 2, 0, 0, 0, 1000.0f, 1.0f, (float*)((uint8_t*)out + 2), out + 16, nullptr) != 0,
           "misaligned colour output");
    // eslam_frame_undistort
    expect(eslam_frame_undistort(rgb, out, 0, 4, rgb + 8, nullptr) != 0, "empty image");
    expect(eslam_frame_undistort(rgb, out, 2, 2, rgb, nullptr) != 0, "in place");
    expect(eslam_frame_undistort(rgb, nullptr, 2, 2, rgb + 8, nullptr) != 0, "null grid");
    expect(eslam_frame_undistort(rgb, out + 1, 2, 2, rgb + 8, nullptr) != 0, "grid not 8-byte aligned");
    if (failures == 0) printf("frame host check ok\n");
    return failures ? 1 : 0;
}
