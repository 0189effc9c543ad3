// tools/convex_fuzz.cpp -- a stand-alone run of opensot_amd/csrc/osot_convex.h over random and degenerate pairs of cores, meant to
// be built with the host compiler's sanitizers (tests/test_convex_shapes_asan_host.py):
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I opensot_amd/csrc tools/convex_fuzz.cpp
// Every result must be finite and stay under the iteration cap; a separated pair must carry its own certificate: the slab
// n . (s_A(-n) - s_B(n)) along n = (ca - cb) / |ca - cb| is a lower bound of the distance and must meet |ca - cb|.
// Usage: convex_fuzz [pairs = 100000] [--hist]   (--hist: the iteration histogram per pair of kinds)
#include <osot_convex.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace osot;

namespace {
uint64_t g_state = 0x9e3779b97f4a7c15ull;
double urand() {      // xorshift64*, uniform in [0, 1)
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) * (1.0 / 9007199254740992.0);
}
double uni(double a, double b) { return a + (b - a) * urand(); }

void random_rotation(double* R) {
    double q[4], n = 0.0;
    do {
        n = 0.0;
        for (int i = 0; i < 4; ++i) { q[i] = uni(-1.0, 1.0); n += q[i] * q[i]; }
    } while (n < 1e-3 || n > 1.0);
    n = 1.0 / sqrt(n);
    const double w = q[0] * n, x = q[1] * n, y = q[2] * n, z = q[3] * n;
    const double M[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                         2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    memcpy(R, M, sizeof(M));
}

struct Shape {
    ConvexCore c;
    std::vector<double> verts;
};

// kind 0 .. 3; degenerate: sizes collapse to zero, vertices repeat
void make_shape(Shape& s, int kind, bool degenerate, double spread) {
    memset(&s.c, 0, sizeof(s.c));
    double R[9];
    random_rotation(R);
    const double p[3] = {uni(-spread, spread), uni(-spread, spread), uni(-spread, spread)};
    const double lo = degenerate ? 0.0 : 0.03;
    if (kind == CVX_SEGMENT) {
        const double h = degenerate && urand() < 0.5 ? 0.0 : uni(lo, 0.3);
        const double e0[3] = {p[0] - h * R[2], p[1] - h * R[5], p[2] - h * R[8]}, e1[3] = {p[0] + h * R[2], p[1] + h * R[5], p[2] + h * R[8]};
        convex_segment(s.c, e0, e1);
        return;
    }
    s.c.kind = kind;
    memcpy(s.c.R, R, sizeof(R));
    memcpy(s.c.p, p, sizeof(p));
    for (int i = 0; i < 3; ++i) s.c.s[i] = (degenerate && urand() < 0.4) ? 0.0 : uni(lo, 0.3);
    if (kind == CVX_HULL) {
        const int nv = 1 + (int)(urand() * kGjkMaxHull) % kGjkMaxHull;
        s.verts.resize(3 * nv);
        for (int k = 0; k < nv; ++k)
            for (int i = 0; i < 3; ++i)
                s.verts[3 * k + i] = (degenerate && k > 0 && urand() < 0.5) ? s.verts[3 * (k - 1) + i] : uni(-0.3, 0.3);
        s.c.v = s.verts.data();
        s.c.nv = nv;
    }
}
}  // namespace

int main(int argc, char** argv) {
    long pairs = 100000;
    bool hist = false;
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--hist")) hist = true;
        else pairs = atol(argv[a]);
    }
    static long H[4][4][kGjkMaxIter + 1];
    long bad = 0, hits = 0, capped = 0;
    double worst = 0.0;
    for (long t = 0; t < pairs; ++t) {
        const int ka = (int)(urand() * 4) & 3, kb = (int)(urand() * 4) & 3;
        const bool degenerate = (t % 4) == 3;
        Shape A, B;
        make_shape(A, ka, degenerate, degenerate ? 0.1 : 0.5);
        make_shape(B, kb, degenerate, degenerate ? 0.1 : 0.5);
        if (degenerate && (t % 16) == 15) memcpy(B.c.p, A.c.p, sizeof(A.c.p));      // coincident centres
        GjkResult r;
        gjk_closest(A.c, B.c, r);
        bool ok = r.iterations >= 0 && r.iterations <= kGjkMaxIter && std::isfinite(r.len) && r.len >= 0.0;
        for (int i = 0; i < 3; ++i) ok = ok && std::isfinite(r.ca[i]) && std::isfinite(r.cb[i]);
        if (ok && !r.intersect && !r.capped) {
            double n[3], m[3], sa[3], sb[3];
            for (int i = 0; i < 3; ++i) { n[i] = (r.ca[i] - r.cb[i]) / r.len; m[i] = -n[i]; }
            convex_support(A.c, m, sa);
            convex_support(B.c, n, sb);
            const double slab = n[0] * (sa[0] - sb[0]) + n[1] * (sa[1] - sb[1]) + n[2] * (sa[2] - sb[2]);
            const double gap = r.len - slab;
            if (gap > worst) worst = gap;
            ok = gap <= 1.0e-9 + 1.0e-9 * r.len && gap >= -1.0e-12;
        }
        hits += r.intersect; capped += r.capped;
        if (ok && r.intersect) ok = r.len == 0.0;
        if (!ok) {
            if (++bad <= 10) fprintf(stderr, "pair %ld (kinds %d %d%s): len %.17g iterations %d intersect %d capped %d\n", t, ka, kb,
                                     degenerate ? ", degenerate" : "", r.len, r.iterations, r.intersect, r.capped);
        }
        H[ka < kb ? ka : kb][ka < kb ? kb : ka][r.iterations]++;
    }
    printf("convex_fuzz: %ld pairs, %ld intersecting, %ld at the iteration cap, worst certificate gap %.3g, %ld failures\n", pairs, hits, capped,
           worst, bad);
    if (hist) {
        static const char* nm[4] = {"segment", "box", "cylinder", "hull"};
        for (int a = 0; a < 4; ++a)
            for (int b = a; b < 4; ++b) {
                printf("%-8s %-8s:", nm[a], nm[b]);
                for (int i = 0; i <= kGjkMaxIter; ++i)
                    if (H[a][b][i]) printf(" %d:%ld", i, H[a][b][i]);
                printf("\n");
            }
    }
    return bad ? 1 : 0;
}
