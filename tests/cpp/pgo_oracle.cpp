// The scalar restatement of the pose-graph optimiser's contract (docs/PGO.md): g2o's VertexSE3 / EdgeSE3 under its
// Levenberg-Marquardt, as graph_slam.cpp:43-49,179-202,332 uses them.  Dense, natural order, sequential sums in edge order,
// a dense scalar Cholesky; BANDED switches the solve to a scalar banded Cholesky under a reverse Cuthill-McKee order, which is
// how tests measure what a change of elimination order alone does to the numbers.  Mutations (a wrong rule behind a switch)
// let tests show that each rule is actually held.  Shares no code with slam_amd/csrc/pgo.hip.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "slam_mi355x.h"

namespace {

typedef std::vector<double> Vec;

enum { MUT_NONE = 0, MUT_LEFT_UPDATE = 1, MUT_NO_FLIP = 2, MUT_SCALE_NO_EPS = 3, MUT_KEEP_LAMBDA = 4 };

struct Iso { // q = (x, y, z, w), t
    double q[4];
    double t[3];
};

void quat_product(const double a[4], const double b[4], double out[4])
{
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    out[0] = aw * bx + bw * ax + (ay * bz - az * by);
    out[1] = aw * by + bw * ay + (az * bx - ax * bz);
    out[2] = aw * bz + bw * az + (ax * by - ay * bx);
    out[3] = aw * bw - (ax * bx + ay * by + az * bz);
}

void rotation(const double q[4], double R[3][3])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0][0] = 1 - 2 * (y * y + z * z), R[0][1] = 2 * (x * y - z * w), R[0][2] = 2 * (x * z + y * w);
    R[1][0] = 2 * (x * y + z * w), R[1][1] = 1 - 2 * (x * x + z * z), R[1][2] = 2 * (y * z - x * w);
    R[2][0] = 2 * (x * z - y * w), R[2][1] = 2 * (y * z + x * w), R[2][2] = 1 - 2 * (x * x + y * y);
}

void rotate(const double q[4], const double v[3], double out[3])
{
    double R[3][3];
    rotation(q, R);
    for (int i = 0; i < 3; ++i) out[i] = R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2];
}

Iso compose(const Iso &a, const Iso &b)
{
    Iso    c;
    double rt[3];
    quat_product(a.q, b.q, c.q);
    rotate(a.q, b.t, rt);
    for (int i = 0; i < 3; ++i) c.t[i] = rt[i] + a.t[i];
    return c;
}

Iso inverse(const Iso &a)
{
    Iso    c;
    double rt[3];
    c.q[0] = -a.q[0], c.q[1] = -a.q[1], c.q[2] = -a.q[2], c.q[3] = a.q[3];
    rotate(c.q, a.t, rt);
    for (int i = 0; i < 3; ++i) c.t[i] = -rt[i];
    return c;
}

// the rule of the ABI: a quaternion already unit to 8 ulp keeps its bits
bool from_pose7(const double p[7], Iso *out)
{
    for (int i = 0; i < 7; ++i)
        if (!std::isfinite(p[i])) return false;
    const double n2 = p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6];
    if (!(n2 > 0)) return false;
    const double div = std::fabs(n2 - 1.0) <= 8 * DBL_EPSILON ? 1.0 : std::sqrt(n2);
    for (int i = 0; i < 3; ++i) out->t[i] = p[i];
    for (int i = 0; i < 4; ++i) out->q[i] = div == 1.0 ? p[3 + i] : p[3 + i] / div;
    return true;
}

Iso from_mqt(const double v[6])
{
    Iso          X;
    const double n2 = v[3] * v[3] + v[4] * v[4] + v[5] * v[5];
    for (int i = 0; i < 3; ++i) X.t[i] = v[i];
    if (n2 > 1) {
        const double n = std::sqrt(n2);
        X.q[0] = v[3] / n, X.q[1] = v[4] / n, X.q[2] = v[5] / n, X.q[3] = 0;
    } else {
        X.q[0] = v[3], X.q[1] = v[4], X.q[2] = v[5], X.q[3] = std::sqrt(1 - n2);
    }
    return X;
}

void to_mqt(const Iso &X, bool flip, double v[6])
{
    const double sign = (flip && X.q[3] < 0) ? -1.0 : 1.0;
    for (int i = 0; i < 3; ++i) v[i] = X.t[i], v[3 + i] = sign * X.q[i];
}

Iso oplus(const Iso &X, const double d[6], bool left)
{
    const Iso D = from_mqt(d);
    Iso       Y = left ? compose(D, X) : compose(X, D);
    const double n = std::sqrt(Y.q[0] * Y.q[0] + Y.q[1] * Y.q[1] + Y.q[2] * Y.q[2] + Y.q[3] * Y.q[3]);
    for (int i = 0; i < 4; ++i) Y.q[i] /= n;
    return Y;
}

struct Edge {
    int    from, to;
    Iso    zinv;
    double W[6][6];
};

struct Graph {
    std::vector<Iso>  X;
    std::vector<char> fixed;
    std::vector<Edge> E;
    int               mutation = MUT_NONE;
    int               max_trials = 10;
    double            tau = 1e-5, lo = 1.0 / 3.0, hi = 2.0 / 3.0;
    double            kept_lambda = 0; // MUT_KEEP_LAMBDA
    bool              have_kept = false;
};

double edge_error(const Graph &G, const std::vector<Iso> &X, const Edge &ed, double e[6])
{
    const Iso D = compose(ed.zinv, compose(inverse(X[ed.from]), X[ed.to]));
    to_mqt(D, G.mutation != MUT_NO_FLIP, e);
    double chi2 = 0;
    for (int r = 0; r < 6; ++r) {
        double we = 0;
        for (int c = 0; c < 6; ++c) we += ed.W[r][c] * e[c];
        chi2 += e[r] * we;
    }
    return chi2;
}

double total_chi2(const Graph &G, const std::vector<Iso> &X)
{
    double sum = 0, e[6];
    for (size_t k = 0; k < G.E.size(); ++k) sum += edge_error(G, X, G.E[k], e);
    return sum;
}

void left_matrix(const double q[4], double M[4][4]) // q (x) p as a matrix on p = (x y z w)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double m[4][4] = {{w, -z, y, x}, {z, w, -x, y}, {-y, x, w, z}, {-x, -y, -z, w}};
    std::memcpy(M, m, sizeof m);
}

void right_matrix(const double q[4], double M[4][4]) // p (x) q as a matrix on p
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double m[4][4] = {{w, z, -y, x}, {-z, w, x, y}, {y, -x, w, z}, {-x, -y, -z, w}};
    std::memcpy(M, m, sizeof m);
}

// the closed forms of docs/PGO.md, built from the 4 x 4 quaternion matrices
void jacobians(const Graph &G, const std::vector<Iso> &X, const Edge &ed, double Ji[6][6], double Jj[6][6])
{
    const Iso &A = ed.zinv;
    const Iso  B = compose(inverse(X[ed.from]), X[ed.to]);
    double     qe[4], Ra[3][3], Rb[3][3], La[4][4], Rmb[4][4], Le[4][4];
    quat_product(A.q, B.q, qe);
    const double s = (G.mutation != MUT_NO_FLIP && qe[3] < 0) ? -1.0 : 1.0;
    rotation(A.q, Ra);
    rotation(B.q, Rb);
    left_matrix(A.q, La);
    right_matrix(B.q, Rmb);
    left_matrix(qe, Le);
    std::memset(Ji, 0, 36 * sizeof(double));
    std::memset(Jj, 0, 36 * sizeof(double));
    const double tbx[3][3] = {{0, -B.t[2], B.t[1]}, {B.t[2], 0, -B.t[0]}, {-B.t[1], B.t[0], 0}};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double re = 0, rx = 0, lr = 0;
            for (int m = 0; m < 3; ++m) re += Ra[r][m] * Rb[m][c], rx += Ra[r][m] * tbx[m][c];
            for (int m = 0; m < 4; ++m) lr += La[r][m] * Rmb[m][c];
            Jj[r][c] = re;
            Jj[3 + r][3 + c] = s * Le[r][c];
            Ji[r][c] = -Ra[r][c];
            Ji[r][3 + c] = 2 * rx;
            Ji[3 + r][3 + c] = -s * lr;
        }
}

// H (6 nv x 6 nv, rows and columns of fixed vertices left zero) and b in vertex numbering, edges in order
void build_system(const Graph &G, const std::vector<Iso> &X, Vec &H, Vec &b)
{
    const size_t n = 6 * X.size();
    H.assign(n * n, 0.0);
    b.assign(n, 0.0);
    for (size_t k = 0; k < G.E.size(); ++k) {
        const Edge &ed = G.E[k];
        double      J[2][6][6], e[6], WJ[2][6][6], We[6];
        jacobians(G, X, ed, J[0], J[1]);
        edge_error(G, X, ed, e);
        const int v[2] = {ed.from, ed.to};
        for (int r = 0; r < 6; ++r) {
            We[r] = 0;
            for (int c = 0; c < 6; ++c) We[r] += ed.W[r][c] * e[c];
            for (int a = 0; a < 2; ++a)
                for (int c = 0; c < 6; ++c) {
                    double s = 0;
                    for (int m = 0; m < 6; ++m) s += ed.W[r][m] * J[a][m][c];
                    WJ[a][r][c] = s;
                }
        }
        for (int a = 0; a < 2; ++a) {
            if (G.fixed[v[a]]) continue;
            for (int r = 0; r < 6; ++r) {
                double g = 0;
                for (int m = 0; m < 6; ++m) g += J[a][m][r] * We[m];
                b[6 * v[a] + r] -= g;
            }
            for (int c2 = 0; c2 < 2; ++c2) {
                if (G.fixed[v[c2]]) continue;
                for (int r = 0; r < 6; ++r)
                    for (int c = 0; c < 6; ++c) {
                        double s = 0;
                        for (int m = 0; m < 6; ++m) s += J[a][m][r] * WJ[c2][m][c];
                        H[(6 * v[a] + r) * n + 6 * v[c2] + c] += s;
                    }
            }
        }
    }
}

// reverse Cuthill-McKee over the free vertices: start at the vertex of least (degree, id) of a component, move to the
// least vertex of the deepest level while that deepens the tree, visit neighbours by (degree, id), reverse everything
void rcm_order(const Graph &G, std::vector<int> &perm, int *w)
{
    const int                     nv = (int)G.X.size();
    std::vector<std::vector<int>> nb(nv);
    for (const Edge &ed : G.E)
        if (!G.fixed[ed.from] && !G.fixed[ed.to]) {
            if (std::find(nb[ed.from].begin(), nb[ed.from].end(), ed.to) == nb[ed.from].end()) {
                nb[ed.from].push_back(ed.to);
                nb[ed.to].push_back(ed.from);
            }
        }
    auto before = [&](int a, int b) { return nb[a].size() != nb[b].size() ? nb[a].size() < nb[b].size() : a < b; };
    std::vector<char> done(nv, 0);
    std::vector<int>  depth(nv, 0);
    auto              walk = [&](int start) {
        std::vector<int>  order(1, start);
        std::vector<char> in(nv, 0);
        in[start] = 1;
        depth[start] = 0;
        for (size_t head = 0; head < order.size(); ++head) {
            std::vector<int> fresh;
            for (int u : nb[order[head]])
                if (!in[u] && !done[u]) {
                    in[u] = 1;
                    depth[u] = depth[order[head]] + 1;
                    fresh.push_back(u);
                }
            std::sort(fresh.begin(), fresh.end(), before);
            for (int u : fresh) order.push_back(u);
        }
        return order;
    };
    perm.clear();
    while (true) {
        int start = -1;
        for (int v = 0; v < nv; ++v)
            if (!G.fixed[v] && !done[v] && (start < 0 || before(v, start))) start = v;
        if (start < 0) break;
        std::vector<int> order = walk(start);
        for (int tries = 0; tries < nv; ++tries) {
            const int deepest = depth[order.back()];
            int       cand = -1;
            for (int v : order)
                if (depth[v] == deepest && (cand < 0 || before(v, cand))) cand = v;
            std::vector<int> other = walk(cand);
            if (depth[other.back()] <= deepest) break;
            order = other;
        }
        for (int v : order) done[v] = 1, perm.push_back(v);
    }
    std::reverse(perm.begin(), perm.end());
    std::vector<int> pos(nv, -1);
    for (size_t r = 0; r < perm.size(); ++r) pos[perm[r]] = (int)r;
    *w = 0;
    for (const Edge &ed : G.E)
        if (pos[ed.from] >= 0 && pos[ed.to] >= 0) *w = std::max(*w, std::abs(pos[ed.from] - pos[ed.to]));
}

// A x = rhs for the free scalars listed in `idx` (their order is the elimination order), by Cholesky on the lower triangle
// with half-bandwidth `hb` (n - 1: dense).  false where a pivot is not positive.
bool solve_spd(const Vec &H, size_t n_all, const Vec &b, double lambda, const std::vector<int> &idx, int hb, Vec &x)
{
    const int n = (int)idx.size();
    Vec       L((size_t)n * n, 0.0), y(n);
    for (int i = 0; i < n; ++i)
        for (int j = std::max(0, i - hb); j <= i; ++j) L[(size_t)i * n + j] = H[(size_t)idx[i] * n_all + idx[j]] + (i == j ? lambda : 0.0);
    for (int j = 0; j < n; ++j) {
        double d = L[(size_t)j * n + j];
        for (int m = std::max(0, j - hb); m < j; ++m) d -= L[(size_t)j * n + m] * L[(size_t)j * n + m];
        if (!(d > 0)) return false;
        d = std::sqrt(d);
        L[(size_t)j * n + j] = d;
        for (int i = j + 1; i <= std::min(n - 1, j + hb); ++i) {
            double v = L[(size_t)i * n + j];
            for (int m = std::max(0, i - hb); m < j; ++m) v -= L[(size_t)i * n + m] * L[(size_t)j * n + m];
            L[(size_t)i * n + j] = v / d;
        }
    }
    for (int i = 0; i < n; ++i) {
        double v = b[idx[i]];
        for (int m = std::max(0, i - hb); m < i; ++m) v -= L[(size_t)i * n + m] * y[m];
        y[i] = v / L[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double v = y[i];
        for (int m = i + 1; m <= std::min(n - 1, i + hb); ++m) v -= L[(size_t)m * n + i] * y[m];
        y[i] = v / L[(size_t)i * n + i];
    }
    x.assign(n_all, 0.0);
    for (int i = 0; i < n; ++i) x[idx[i]] = y[i];
    return true;
}

struct Trial {
    Vec              delta;
    std::vector<Iso> cand;
    double           chi2_cand, scale;
    bool             pivot;
};

void solve_trial(const Graph &G, const std::vector<Iso> &X, const Vec &H, const Vec &b, double lambda, bool banded, Trial &T)
{
    std::vector<int> idx;
    int              hb;
    if (banded) {
        std::vector<int> perm;
        int              w = 0;
        rcm_order(G, perm, &w);
        for (int v : perm)
            for (int c = 0; c < 6; ++c) idx.push_back(6 * v + c);
        hb = 6 * w + 5;
    } else {
        for (size_t v = 0; v < X.size(); ++v)
            if (!G.fixed[v])
                for (int c = 0; c < 6; ++c) idx.push_back(6 * (int)v + c);
        hb = std::max(0, (int)idx.size() - 1);
    }
    T.pivot = !solve_spd(H, b.size(), b, lambda, idx, hb, T.delta);
    if (T.pivot) T.delta.assign(b.size(), 0.0);
    T.scale = 0;
    if (!T.pivot)
        for (int k : idx) T.scale += T.delta[k] * (lambda * T.delta[k] + b[k]);
    T.cand = X;
    for (size_t v = 0; v < X.size(); ++v)
        if (!G.fixed[v]) T.cand[v] = oplus(X[v], &T.delta[6 * v], G.mutation == MUT_LEFT_UPDATE);
    T.chi2_cand = total_chi2(G, T.cand);
}

} // namespace

extern "C" {

void *pgoo_create() { return new Graph; }
void  pgoo_destroy(void *h) { delete static_cast<Graph *>(h); }
void  pgoo_set_mutation(void *h, int m) { static_cast<Graph *>(h)->mutation = m; }
void  pgoo_set_params(void *h, int max_trials, double tau, double lo, double hi)
{
    Graph *G = static_cast<Graph *>(h);
    G->max_trials = max_trials, G->tau = tau, G->lo = lo, G->hi = hi;
}

int pgoo_add_vertex(void *h, const double *pose, int fixed)
{
    Graph *G = static_cast<Graph *>(h);
    Iso    X;
    if (!from_pose7(pose, &X)) return -1;
    G->X.push_back(X);
    G->fixed.push_back(fixed ? 1 : 0);
    return 0;
}

int pgoo_set_vertex(void *h, int id, const double *pose)
{
    Graph *G = static_cast<Graph *>(h);
    Iso    X;
    if (id < 0 || id >= (int)G->X.size() || !from_pose7(pose, &X)) return -1;
    G->X[id] = X;
    return 0;
}

int pgoo_add_edge(void *h, int from, int to, const double *meas, const double *info)
{
    Graph *G = static_cast<Graph *>(h);
    Edge   ed;
    Iso    Z;
    if (from < 0 || to < 0 || from >= (int)G->X.size() || to >= (int)G->X.size() || from == to || !from_pose7(meas, &Z)) return -1;
    ed.from = from, ed.to = to, ed.zinv = inverse(Z);
    std::memcpy(ed.W, info, sizeof ed.W);
    G->E.push_back(ed);
    return 0;
}

void pgoo_read_vertices(void *h, double *out)
{
    Graph *G = static_cast<Graph *>(h);
    for (size_t v = 0; v < G->X.size(); ++v) {
        const double sign = G->X[v].q[3] < 0 ? -1.0 : 1.0;
        for (int i = 0; i < 3; ++i) out[7 * v + i] = G->X[v].t[i];
        for (int i = 0; i < 4; ++i) out[7 * v + 3 + i] = sign * G->X[v].q[i];
    }
}

// e (6 per edge) and chi2 per edge, each nullable; returns the sum in edge order
double pgoo_chi2(void *h, double *e_out, double *chi2_e)
{
    Graph *G = static_cast<Graph *>(h);
    double sum = 0, e[6];
    for (size_t k = 0; k < G->E.size(); ++k) {
        const double c = edge_error(*G, G->X, G->E[k], e);
        if (e_out) std::memcpy(e_out + 6 * k, e, sizeof e);
        if (chi2_e) chi2_e[k] = c;
        sum += c;
    }
    return sum;
}

void pgoo_jacobians(void *h, int edge, double *Ji, double *Jj)
{
    Graph *G = static_cast<Graph *>(h);
    double a[6][6], b[6][6];
    jacobians(*G, G->X, G->E[edge], a, b);
    std::memcpy(Ji, a, sizeof a);
    std::memcpy(Jj, b, sizeof b);
}

void pgoo_system(void *h, double *H, double *b)
{
    Graph *G = static_cast<Graph *>(h);
    Vec    Hv, bv;
    build_system(*G, G->X, Hv, bv);
    std::copy(Hv.begin(), Hv.end(), H);
    std::copy(bv.begin(), bv.end(), b);
}

int pgoo_rcm(void *h, int *perm, int *w)
{
    Graph           *G = static_cast<Graph *>(h);
    std::vector<int> p;
    rcm_order(*G, p, w);
    std::copy(p.begin(), p.end(), perm);
    return (int)p.size();
}

// one trial at lambda, applying nothing; out[4] = chi2 before, chi2 after, scale (without the 1e-3), pivot flag
void pgoo_step(void *h, double lambda, int banded, double *delta, double *out)
{
    Graph *G = static_cast<Graph *>(h);
    Vec    H, b;
    Trial  T;
    build_system(*G, G->X, H, b);
    solve_trial(*G, G->X, H, b, lambda, banded != 0, T);
    if (delta) std::copy(T.delta.begin(), T.delta.end(), delta);
    out[0] = total_chi2(*G, G->X), out[1] = T.chi2_cand, out[2] = T.scale, out[3] = T.pivot ? 1.0 : 0.0;
}

// optimize(n).  margins (nullable, SLAM_PGO_TRACE doubles): |chi2 - chi2'| / chi2 of every traced trial, for MARGIN_TOL.
int pgoo_optimize(void *h, int iterations, int banded, slam_pgo_result *res, double *margins)
{
    Graph *G = static_cast<Graph *>(h);
    bool   any_fixed = false;
    for (char f : G->fixed) any_fixed = any_fixed || f;
    if (!any_fixed) return SLAM_E_INVALID;
    slam_pgo_result R;
    std::memset(&R, 0, sizeof R);
    R.stop_reason = SLAM_PGO_STOP_ITERATIONS;
    double chi2 = total_chi2(*G, G->X), lambda = 0, nu = 2;
    R.chi2_initial = chi2;
    int n_free = 0;
    for (char f : G->fixed) n_free += !f;
    R.free_vertices = n_free;
    for (int it = 0; it < iterations && n_free > 0; ++it) {
        Vec H, b;
        build_system(*G, G->X, H, b);
        if (it == 0) {
            if (G->mutation == MUT_KEEP_LAMBDA && G->have_kept)
                lambda = G->kept_lambda;
            else {
                double      top = 0;
                bool        first = true;
                const size_t n = b.size();
                for (size_t v = 0; v < G->X.size(); ++v)
                    if (!G->fixed[v])
                        for (int c = 0; c < 6; ++c) {
                            const double d = H[(6 * v + c) * n + 6 * v + c];
                            top = first ? d : std::max(top, d);
                            first = false;
                        }
                lambda = G->tau * top;
            }
            nu = 2;
        }
        double rho = 0;
        int    trials = 0;
        chi2 = total_chi2(*G, G->X);
        do {
            Trial T;
            solve_trial(*G, G->X, H, b, lambda, banded != 0, T);
            const double cand = T.pivot ? DBL_MAX : T.chi2_cand;
            const double scale = T.scale + (G->mutation == MUT_SCALE_NO_EPS ? 0.0 : 1e-3);
            rho = (chi2 - cand) / scale;
            const bool accept = rho > 0 && std::isfinite(cand);
            if (R.n_trials < SLAM_PGO_TRACE) {
                slam_pgo_trial &t = R.trace[R.n_trials];
                t.lambda = lambda, t.rho = rho, t.chi2 = cand, t.accepted = accept, t.reserved = 0;
                if (margins) margins[R.n_trials] = std::fabs(chi2 - cand) / chi2;
            }
            ++R.n_trials;
            if (accept) {
                double alpha = 1 - std::pow(2 * rho - 1, 3);
                alpha = std::min(alpha, G->hi);
                lambda *= std::max(G->lo, alpha);
                nu = 2;
                chi2 = cand;
                G->X = T.cand;
            } else {
                lambda *= nu;
                nu *= 2;
            }
            ++trials;
        } while (rho < 0 && trials < G->max_trials);
        ++R.iterations;
        if (trials == G->max_trials || rho == 0) {
            R.stop_reason = trials == G->max_trials ? SLAM_PGO_STOP_MAX_TRIALS : SLAM_PGO_STOP_RHO_ZERO;
            break;
        }
    }
    G->kept_lambda = lambda, G->have_kept = true;
    R.chi2_final = chi2;
    if (res) *res = R;
    return SLAM_OK;
}

// the vector maps, for the round-trip tests
void pgoo_from_mqt(const double *v, double *pose7)
{
    const Iso X = from_mqt(v);
    for (int i = 0; i < 3; ++i) pose7[i] = X.t[i];
    for (int i = 0; i < 4; ++i) pose7[3 + i] = X.q[i];
}

void pgoo_to_mqt(const double *pose7, int flip, double *v)
{
    Iso X;
    for (int i = 0; i < 3; ++i) X.t[i] = pose7[i];
    for (int i = 0; i < 4; ++i) X.q[i] = pose7[3 + i];
    to_mqt(X, flip != 0, v);
}

void pgoo_oplus(const double *pose7, const double *delta, int left, double *out7)
{
    Iso X;
    for (int i = 0; i < 3; ++i) X.t[i] = pose7[i];
    for (int i = 0; i < 4; ++i) X.q[i] = pose7[3 + i];
    const Iso Y = oplus(X, delta, left != 0);
    for (int i = 0; i < 3; ++i) out7[i] = Y.t[i];
    for (int i = 0; i < 4; ++i) out7[3 + i] = Y.q[i];
}

void pgoo_compose(const double *a7, const double *b7, double *out7)
{
    Iso A, B;
    for (int i = 0; i < 3; ++i) A.t[i] = a7[i], B.t[i] = b7[i];
    for (int i = 0; i < 4; ++i) A.q[i] = a7[3 + i], B.q[i] = b7[3 + i];
    const Iso Y = compose(A, B);
    for (int i = 0; i < 3; ++i) out7[i] = Y.t[i];
    for (int i = 0; i < 4; ++i) out7[3 + i] = Y.q[i];
}

} // extern "C"
