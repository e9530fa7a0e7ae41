// csm_oracle.cpp -- scalar, single-threaded restatement of the correlative scan matcher's contract (docs/CSM.md): the
// tables, the exhaustive score volume and the two-level search.  slam_csm_* is held to it bit for bit.  Built by
// tests/csm_oracle.py with g++ -O2 -ffp-contract=off (every product and every sum rounded on its own).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "slam_mi355x.h"

namespace {

const double kCellLimit = 1073741824.0; // 2^30

bool cell_of(double v, double res, int32_t &c)
{
    const double f = std::floor(v / res);
    if (!(std::fabs(f) <= kCellLimit)) return false; // NaN, infinite or beyond the lattice
    c = (int32_t)f;
    return true;
}

struct Table {
    int                  ox = 0, oy = 0, w = 0, h = 0; // window of the lattice; w = h = 0: no table
    std::vector<uint8_t> v;
    int at(long long u, long long vv) const
    {
        const long long i = u - ox, j = vv - oy;
        return (i < 0 || j < 0 || i >= w || j >= h) ? 0 : v[(size_t)j * w + i];
    }
};

struct Oracle {
    slam_csm_params P;
    int             K, D;
    Table           T[2], W[2];
    int nth() const { return 2 * P.half_theta + 1; }
    int nx() const { return 2 * P.half_x + 1; }
    int ny() const { return 2 * P.half_y + 1; }
    int nbx() const { return (nx() + D - 1) / D; }
    int nby() const { return (ny() + D - 1) / D; }
};

void build_tables(Oracle &o, int c, const double *m, int n)
{
    if (n <= 3) return; // icpPointToPoint.cpp:59,93
    const int            K = o.K, S = 2 * K + 1, D = o.D;
    std::vector<uint8_t> stamp((size_t)S * S);
    for (int j = 0; j < S; ++j)
        for (int i = 0; i < S; ++i) {
            const double d2 = (double)((i - K) * (i - K) + (j - K) * (j - K));
            stamp[(size_t)j * S + i] = (uint8_t)std::rint(255.0 * std::exp(-(d2 * (o.P.resolution * o.P.resolution)) / (2.0 * (o.P.sigma * o.P.sigma))));
        }
    std::vector<int32_t> cx, cy;
    for (int i = 0; i < n; ++i) {
        int32_t a, b;
        if (cell_of(m[2 * i], o.P.resolution, a) && cell_of(m[2 * i + 1], o.P.resolution, b)) cx.push_back(a), cy.push_back(b);
    }
    if (cx.empty()) return;
    int32_t x0 = cx[0], x1 = cx[0], y0 = cy[0], y1 = cy[0];
    for (size_t i = 0; i < cx.size(); ++i) {
        x0 = cx[i] < x0 ? cx[i] : x0, x1 = cx[i] > x1 ? cx[i] : x1;
        y0 = cy[i] < y0 ? cy[i] : y0, y1 = cy[i] > y1 ? cy[i] : y1;
    }
    Table &T = o.T[c];
    T.ox = x0 - K, T.oy = y0 - K, T.w = x1 - x0 + 1 + 2 * K, T.h = y1 - y0 + 1 + 2 * K;
    T.v.assign((size_t)T.w * T.h, 0);
    for (size_t p = 0; p < cx.size(); ++p)
        for (int j = 0; j < S; ++j)
            for (int i = 0; i < S; ++i) {
                uint8_t &t = T.v[(size_t)(cy[p] + j - K - T.oy) * T.w + (cx[p] + i - K - T.ox)];
                if (stamp[(size_t)j * S + i] > t) t = stamp[(size_t)j * S + i];
            }
    Table &W = o.W[c];
    W.ox = T.ox - (D - 1), W.oy = T.oy - (D - 1), W.w = T.w + D - 1, W.h = T.h + D - 1;
    W.v.assign((size_t)W.w * W.h, 0);
    for (int v = 0; v < W.h; ++v)
        for (int u = 0; u < W.w; ++u) {
            int best = 0;
            for (int j = 0; j < D; ++j)
                for (int i = 0; i < D; ++i) {
                    const int t = T.at((long long)W.ox + u + i, (long long)W.oy + v + j);
                    best = t > best ? t : best;
                }
            W.v[(size_t)v * W.w + u] = (uint8_t)best;
        }
}

void angles(const Oracle &o, const double R0[4], double *cs)
{
    const double th0 = std::atan2(R0[2], R0[0]);
    for (int k = 0; k < o.nth(); ++k) {
        const double th = th0 + (double)(k - o.P.half_theta) * o.P.theta_step;
        cs[2 * k] = std::cos(th), cs[2 * k + 1] = std::sin(th);
    }
}

// the cells of one scan at one angle: class (-1 = not counted), cell
struct Cells {
    std::vector<int>     cls;
    std::vector<int32_t> cx, cy;
    int                  counted = 0;
};

Cells cells_at(const Oracle &o, const double *pts, int n, int n_ga, double c, double s, const double t0[2])
{
    Cells out;
    out.cls.assign(n, -1), out.cx.assign(n, 0), out.cy.assign(n, 0);
    for (int i = 0; i < n; ++i) {
        const int    cl = i < n_ga ? 0 : 1;
        const double px = pts[2 * i], py = pts[2 * i + 1];
        const double qx = (c * px - s * py) + t0[0], qy = (s * px + c * py) + t0[1];
        int32_t      a, b;
        if (o.T[cl].w == 0 || !cell_of(qx, o.P.resolution, a) || !cell_of(qy, o.P.resolution, b)) continue;
        out.cls[i] = cl, out.cx[i] = a, out.cy[i] = b;
        ++out.counted;
    }
    return out;
}

int32_t score_at(const Oracle &o, const Cells &q, int a, int b)
{
    int32_t s = 0;
    for (size_t i = 0; i < q.cls.size(); ++i)
        if (q.cls[i] >= 0) s += o.T[q.cls[i]].at((long long)q.cx[i] + (a - o.P.half_x), (long long)q.cy[i] + (b - o.P.half_y));
    return s;
}

int32_t bound_at(const Oracle &o, const Cells &q, int A, int B)
{
    int32_t s = 0;
    for (size_t i = 0; i < q.cls.size(); ++i)
        if (q.cls[i] >= 0) s += o.W[q.cls[i]].at((long long)q.cx[i] + (A * o.D - o.P.half_x), (long long)q.cy[i] + (B * o.D - o.P.half_y));
    return s;
}

struct Best {
    long long score = -1;
    long long flat = 0;
    void      offer(long long s, long long f)
    {
        if (s > score || (s == score && f < flat)) score = s, flat = f;
    }
};

void eval_block(const Oracle &o, const Cells &q, int k, int A, int B, Best &best)
{
    for (int j = 0; j < o.D; ++j)
        for (int i = 0; i < o.D; ++i) {
            const int a = A * o.D + i, b = B * o.D + j;
            if (a < o.nx() && b < o.ny()) best.offer(score_at(o, q, a, b), ((long long)k * o.ny() + b) * o.nx() + a);
        }
}

} // namespace

extern "C" {

void *csmo_create(const double *m_ga, int n_ga, const double *m_nga, int n_nga, const slam_csm_params *p)
{
    Oracle *o = new Oracle();
    o->P = *p;
    o->K = p->kernel_cells > 0 ? p->kernel_cells : (int)std::ceil(3.0 * p->sigma / p->resolution - 1e-9);
    o->P.kernel_cells = o->K;
    o->D = p->block;
    build_tables(*o, 0, m_ga, n_ga);
    build_tables(*o, 1, m_nga, n_nga);
    return o;
}

void csmo_destroy(void *h) { delete static_cast<Oracle *>(h); }

void csmo_set_window(void *h, int half_x, int half_y, int half_theta, double theta_step)
{
    Oracle *o = static_cast<Oracle *>(h);
    o->P.half_x = half_x, o->P.half_y = half_y, o->P.half_theta = half_theta, o->P.theta_step = theta_step;
}

int csmo_kernel_cells(void *h) { return static_cast<Oracle *>(h)->K; }

void csmo_table(void *h, int cls, int level, int *ox, int *oy, int *w, int *hh, uint8_t *buf)
{
    const Oracle *o = static_cast<Oracle *>(h);
    const Table  &t = level ? o->W[cls] : o->T[cls];
    *ox = t.ox, *oy = t.oy, *w = t.w, *hh = t.h;
    if (buf && !t.v.empty()) std::memcpy(buf, t.v.data(), t.v.size());
}

void csmo_angles(void *h, const double R0[4], double *cs) { angles(*static_cast<Oracle *>(h), R0, cs); }

// every S(k, b, a), and (optional) the points counted per angle
void csmo_volume(void *h, const double *pts, int n, int n_ga, const double R0[4], const double t0[2], int32_t *vol, int32_t *counted)
{
    const Oracle       &o = *static_cast<Oracle *>(h);
    std::vector<double> cs(2 * (size_t)o.nth());
    angles(o, R0, cs.data());
    for (int k = 0; k < o.nth(); ++k) {
        const Cells q = cells_at(o, pts, n, n_ga, cs[2 * k], cs[2 * k + 1], t0);
        if (counted) counted[k] = q.counted;
        for (int b = 0; b < o.ny(); ++b)
            for (int a = 0; a < o.nx(); ++a) vol[((size_t)k * o.ny() + b) * o.nx() + a] = score_at(o, q, a, b);
    }
}

// every U(k, B, A)
void csmo_bounds(void *h, const double *pts, int n, int n_ga, const double R0[4], const double t0[2], int32_t *U)
{
    const Oracle       &o = *static_cast<Oracle *>(h);
    std::vector<double> cs(2 * (size_t)o.nth());
    angles(o, R0, cs.data());
    for (int k = 0; k < o.nth(); ++k) {
        const Cells q = cells_at(o, pts, n, n_ga, cs[2 * k], cs[2 * k + 1], t0);
        for (int B = 0; B < o.nby(); ++B)
            for (int A = 0; A < o.nbx(); ++A) U[((size_t)k * o.nby() + B) * o.nbx() + A] = bound_at(o, q, A, B);
    }
}

// the answer: exhaustive != 0 evaluates every block, else the two-level search.  R, t in/out.
void csmo_match(void *h, const double *pts, int n, int n_ga, double R[4], double t[2], int exhaustive, slam_csm_result *res)
{
    const Oracle &o = *static_cast<Oracle *>(h);
    std::memset(res, 0, sizeof *res);
    if (n < 5) {
        res->score = -1;
        return;
    }
    const int           nb = o.nbx() * o.nby();
    std::vector<double> cs(2 * (size_t)o.nth());
    angles(o, R, cs.data());
    std::vector<Cells> q;
    for (int k = 0; k < o.nth(); ++k) q.push_back(cells_at(o, pts, n, n_ga, cs[2 * k], cs[2 * k + 1], t));
    Best best;
    int  evaluated = 0;
    if (exhaustive) {
        for (int k = 0; k < o.nth(); ++k)
            for (int c = 0; c < nb; ++c) eval_block(o, q[k], k, c % o.nbx(), c / o.nbx(), best), ++evaluated;
    } else {
        std::vector<int32_t> U((size_t)o.nth() * nb);
        size_t               top = 0;
        for (int k = 0; k < o.nth(); ++k)
            for (int c = 0; c < nb; ++c) {
                const size_t f = (size_t)k * nb + c;
                U[f] = bound_at(o, q[k], c % o.nbx(), c / o.nbx());
                if (U[f] > U[top]) top = f;
            }
        eval_block(o, q[top / nb], (int)(top / nb), (int)(top % nb) % o.nbx(), (int)(top % nb) / o.nbx(), best), ++evaluated;
        const long long L = best.score;
        for (size_t f = 0; f < U.size(); ++f)
            if (f != top && U[f] >= L) eval_block(o, q[f / nb], (int)(f / nb), (int)(f % nb) % o.nbx(), (int)(f % nb) / o.nbx(), best), ++evaluated;
    }
    res->k = (int)(best.flat / ((long long)o.nx() * o.ny()));
    res->b = (int)(best.flat / o.nx() % o.ny());
    res->a = (int)(best.flat % o.nx());
    res->score = (int)best.score;
    res->n_points = q[res->k].counted;
    res->max_score = 255 * res->n_points;
    res->blocks_evaluated = evaluated;
    const double c = cs[2 * res->k], s = cs[2 * res->k + 1];
    R[0] = c, R[1] = -s, R[2] = s, R[3] = c;
    t[0] = t[0] + (double)(res->a - o.P.half_x) * o.P.resolution;
    t[1] = t[1] + (double)(res->b - o.P.half_y) * o.P.resolution;
}

} // extern "C"
