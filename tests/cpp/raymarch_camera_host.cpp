// raymarch_camera_host.cpp -- the camera arithmetic of the C++ host layer (include/SdfKit.hpp: Matrix4x4::CreateLookAt,
// CreatePerspectiveFieldOfView, operator*, Invert and RayMarcher::Camera) on the CPU, for tests/test_raymarch.py to compare bit for
// bit with the oracle's orc_ray_camera.  No GPU call is made: an Sdf is only lowered when it is rendered.
//
// stdin: one case per line, 14 words: the bits (hex) of position[3], target[3], up[3], field of view in degrees, near, far, then
// width and height (decimal).  stdout: per case one line of 19 hex words: the bits of the camera position[3] and of the inverse
// view-projection[16], row-major.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "SdfKit.hpp"

using namespace SdfKit;

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main()
{
    const Sdf sdf = Sdfs::Sphere(1.0f);
    uint32_t b[12];
    int w, h, cases = 0;
    for (;;) {
        int got = 0;
        for (int q = 0; q < 12; q++) got += scanf("%" SCNx32, &b[q]) == 1;
        if (got == 0) break;
        if (got != 12 || scanf("%d %d", &w, &h) != 2) { fprintf(stderr, "bad case line\n"); return 2; }
        float v[12];
        for (int q = 0; q < 12; q++) v[q] = from_bits(b[q]);
        RayMarcher rm(w, h, sdf);
        rm.ViewTransform = Matrix4x4::CreateLookAt(Vector3(v[0], v[1], v[2]), Vector3(v[3], v[4], v[5]), Vector3(v[6], v[7], v[8]));
        rm.VerticalFieldOfViewDegrees = v[9];
        rm.NearPlaneDistance = v[10];
        rm.FarPlaneDistance = v[11];
        float pos[3];
        Matrix4x4 vpi;
        rm.Camera(pos, vpi);
        for (int q = 0; q < 3; q++) printf("%08" PRIx32 " ", to_bits(pos[q]));
        for (int q = 0; q < 16; q++) printf("%08" PRIx32 "%c", to_bits(vpi.M[q / 4][q % 4]), q == 15 ? '\n' : ' ');
        cases++;
    }
    fprintf(stderr, "raymarch_camera_host: %d cases\n", cases);
    return 0;
}
