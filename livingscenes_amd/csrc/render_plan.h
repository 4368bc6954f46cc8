// render_plan.h -- the integer part of the depth renderer (meshrender.hip), the one statement of it: the snap of a projected corner to 1/256
// pixel, the pixel box of a face clipped to the image (floor / ceil division that is right for negative integers), the edge functions, the
// rule that sends a face to the per-thread or to the per-wave rasteriser, the rule that cuts the image into strips for the large faces of a
// call with few items, and the layout of the workspace.  Pure functions: no HIP, no global state.  The kernels call them on the device; a plain C++17 compiler accepts the file, and tests/test_render_cpu.py replays it against the
// NumPy twin of the definition (tests/render_oracle.py; the definition itself: include/livingscenes_hip.h, ls_mesh_render_depth_f64).
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define LS_RP_HD __host__ __device__ inline
#else
#define LS_RP_HD inline
#endif

namespace ls {
namespace rp {

constexpr int RENDER_SUB = 256;                          // sub-pixel positions per pixel
constexpr long long RENDER_SNAP_MAX = 1ll << 24;         // largest |snapped coordinate|: every edge function stays below 2^53, exact as a double
constexpr int RENDER_SMALL_BOX = 64;                     // a face whose clipped box has at most this many pixels is rasterised by its own thread

// floor(a / 256), ceil(a / 256) for any sign (an arithmetic shift rounds down)
LS_RP_HD long long floor_div_sub(long long a) { return a >> 8; }
LS_RP_HD long long ceil_div_sub(long long a) { return -((-a) >> 8); }

// step 4: (int64) floor(u * 256 + 0.5); false when the value is not finite or exceeds 2^24 in magnitude
LS_RP_HD bool snap(double u, long long* out) {
    const double t = floor(u * (double)RENDER_SUB + 0.5);
    if (!(fabs(t) <= (double)RENDER_SNAP_MAX)) return false;   // NaN fails the comparison
    *out = (long long)t;
    return true;
}

struct Box { int x0, x1, y0, y1; };   // pixels [x0, x1] x [y0, y1]; empty when x0 > x1 or y0 > y1

// step 5: the pixels whose centres can lie in the face, clipped to the W x H image
LS_RP_HD Box pixel_box(const long long (&xs)[3], const long long (&ys)[3], int W, int H) {
    long long xmin = xs[0], xmax = xs[0], ymin = ys[0], ymax = ys[0];
    for (int i = 1; i < 3; ++i) {
        xmin = xs[i] < xmin ? xs[i] : xmin;
        xmax = xs[i] > xmax ? xs[i] : xmax;
        ymin = ys[i] < ymin ? ys[i] : ymin;
        ymax = ys[i] > ymax ? ys[i] : ymax;
    }
    long long x0 = ceil_div_sub(xmin), x1 = floor_div_sub(xmax), y0 = ceil_div_sub(ymin), y1 = floor_div_sub(ymax);
    x0 = x0 < 0 ? 0 : x0;
    y0 = y0 < 0 ? 0 : y0;
    x1 = x1 > W - 1 ? W - 1 : x1;
    y1 = y1 > H - 1 ? H - 1 : y1;
    if (x0 > x1 || y0 > y1) return {0, -1, 0, -1};
    return {(int)x0, (int)x1, (int)y0, (int)y1};
}

LS_RP_HD bool box_empty(const Box& b) { return b.x0 > b.x1 || b.y0 > b.y1; }
LS_RP_HD long long box_pixels(const Box& b) { return box_empty(b) ? 0 : (long long)(b.x1 - b.x0 + 1) * (b.y1 - b.y0 + 1); }
// the small / large rule: true = the face's own thread walks the box, false = the 64 lanes of its wave walk it together
LS_RP_HD bool box_small(const Box& b) { return box_pixels(b) <= RENDER_SMALL_BOX; }

// Who walks the large boxes.  With many (view, face) items the rasteriser's waves walk their own large faces (count == 1): the chip is full
// anyway.  With few items -- a handful of faces over a big image -- one wave would walk whole images alone, so the image is cut into
// `count` strips of `rows` rows and a second pass gives every (wave of 64 items, strip) pair its own wave, which repeats steps 1 - 5 for
// its items: about RENDER_STRIP_WAVES waves in all, strips of at least RENDER_STRIP_MIN_ROWS rows.  A choice of speed alone: a pixel's
// key is the same minimum whoever offers the candidates.
constexpr int RENDER_STRIP_WAVES = 1024;
constexpr int RENDER_STRIP_MIN_ROWS = 4;
constexpr int RENDER_MAX_STRIPS = 65535;                 // a grid's y extent
struct Strips { int count, rows; };
LS_RP_HD Strips render_strips(long long items, int H) {
    long long waves = (items + 63) / 64;
    waves = waves < 1 ? 1 : waves;
    long long s = RENDER_STRIP_WAVES / waves, smax = H / RENDER_STRIP_MIN_ROWS;
    smax = smax > RENDER_MAX_STRIPS ? RENDER_MAX_STRIPS : smax;
    s = s > smax ? smax : s;
    s = s < 1 ? 1 : s;
    const int rows = (int)((H + s - 1) / s);
    return {(H + rows - 1) / rows, rows};
}

// step 6: edge(i, j) at the sub-pixel position (X, Y)
LS_RP_HD long long edge(const long long (&xs)[3], const long long (&ys)[3], int i, int j, long long X, long long Y) {
    return (xs[j] - xs[i]) * (Y - ys[i]) - (ys[j] - ys[i]) * (X - xs[i]);
}
// A = e0 + e1 + e2: twice the signed area of the snapped triangle, the same at every pixel
LS_RP_HD long long area2(const long long (&xs)[3], const long long (&ys)[3]) {
    return edge(xs, ys, 1, 2, 0, 0) + edge(xs, ys, 2, 0, 0, 0) + edge(xs, ys, 0, 1, 0, 0);
}
LS_RP_HD bool covered(long long e0, long long e1, long long e2) {
    return e0 + e1 + e2 != 0 && ((e0 >= 0 && e1 >= 0 && e2 >= 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0));
}

// step 7: nearest depth wins, on equal fp32 depth the lower face index (d > 0: its bits order like the floats)
constexpr unsigned long long RENDER_NO_KEY = ~0ull;
LS_RP_HD unsigned long long pixel_key(unsigned depth_bits, int face) { return ((unsigned long long)depth_bits << 32) | (unsigned)face; }

// the workspace of a render call as byte offsets: it depends on (views, H, W, M) alone.  n_off_arrays: the int64 arrays of M + 1 entries a
// batch uploads (0: one mesh).  Pieces start on multiples of 256 bytes, as ls_workspace.h cuts them.
struct RenderLayout { size_t offs = 0, keys = 0, bytes = 0; };
LS_RP_HD size_t rp_align(size_t x) { return (x + 255) & ~(size_t)255; }
LS_RP_HD RenderLayout render_layout(long long views, int H, int W, int M, int n_off_arrays) {
    RenderLayout l;
    l.offs = 0;
    l.keys = rp_align((size_t)n_off_arrays * (size_t)(M + 1) * sizeof(long long));
    l.bytes = rp_align(l.keys + (size_t)views * (size_t)H * (size_t)W * sizeof(unsigned long long));
    return l;
}

}  // namespace rp
}  // namespace ls
