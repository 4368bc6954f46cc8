// render_plan_dump -- csrc/render_plan.h compiled on its own with the host compiler, for tests/test_render_cpu.py.
// stdin, one case per line:  W H u0 v0 u1 v1 u2 v2   (the projected corners as C99 hexadecimal doubles)
// stdout, one line per case: ok xs0 ys0 xs1 ys1 xs2 ys2 A x0 x1 y0 y1 pixels small    (ok = 0: a snap was refused, the rest is 0)
// A line "constants" answers: RENDER_SUB RENDER_SNAP_MAX RENDER_SMALL_BOX RENDER_STRIP_WAVES RENDER_STRIP_MIN_ROWS RENDER_MAX_STRIPS
// A line "strips ITEMS H" answers: count rows   (render_strips)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "render_plan.h"

int main() {
    using namespace ls::rp;
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "constants", 9)) {
            printf("%d %lld %d %d %d %d\n", RENDER_SUB, RENDER_SNAP_MAX, RENDER_SMALL_BOX, RENDER_STRIP_WAVES, RENDER_STRIP_MIN_ROWS, RENDER_MAX_STRIPS);
            continue;
        }
        if (!strncmp(line, "strips", 6)) {
            char* q = line + 6;
            const long long items = strtoll(q, &q, 10);
            const Strips st = render_strips(items, (int)strtol(q, &q, 10));
            printf("%d %d\n", st.count, st.rows);
            continue;
        }
        char* p = line;
        const int W = (int)strtol(p, &p, 10), H = (int)strtol(p, &p, 10);
        double uv[6];
        for (double& t : uv) t = strtod(p, &p);
        long long xs[3] = {0, 0, 0}, ys[3] = {0, 0, 0};
        bool ok = true;
        for (int i = 0; i < 3; ++i) {
            ok = snap(uv[2 * i], &xs[i]) && ok;
            ok = snap(uv[2 * i + 1], &ys[i]) && ok;
        }
        if (!ok) {
            printf("0 0 0 0 0 0 0 0 0 0 0 0 0 0\n");
            continue;
        }
        const Box b = pixel_box(xs, ys, W, H);
        printf("1 %lld %lld %lld %lld %lld %lld %lld %d %d %d %d %lld %d\n", xs[0], ys[0], xs[1], ys[1], xs[2], ys[2], area2(xs, ys), b.x0, b.x1, b.y0,
               b.y1, box_pixels(b), box_small(b) ? 1 : 0);
    }
    return 0;
}
