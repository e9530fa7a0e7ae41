// pf.hip -- Monte Carlo localisation over a grid matcher (slam_pf_*, docs/PARTICLE_FILTER.md): a particle filter whose
// likelihood step is slam_csm_score_poses_dev as it stands.
//
// predict is one launch over the particles (three table-Gaussian draws from Philox-4x32-10 and a rigid motion) and one
// one-thread launch that advances the step counter.  update is the scorer between six launches of its own on the caller's
// stream and no host wait: the poses, acc += score with the maximum, the weights with their integer sums and a block scan,
// the decision with the scan of the block sums, a binary search per output that gathers into a second buffer, and the copy
// back.  The decision is made on the device and read there: a launch that finds it negative returns at once, so no host
// pointer depends on it and a captured graph replays either way.  Sums are integer atomics (the same bits in any order); there
// is no wait between workgroups anywhere: what one launch needs of another is ordered by the stream.
// The floating-point steps are spelled with __dmul_rn / __dadd_rn; cos, sin, the Gaussian quantiles and the weights come
// from the host (pf_tables.hpp).
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "common.hpp"
#include "device_mem.hpp"
#include "pf_tables.hpp"

using namespace slam;

namespace {

constexpr int      kBlock = 256;            // threads of every launch over the particles, and items of one scan block
constexpr int      kMaxParticles = 1 << 18; // so that every integer sum fits 64 bits (slam_mi355x.h)
constexpr int      kMaxWords = 1 << 20;
constexpr double   kStepLimit = 1048576.0; // 2^20: sk and |dk| stay below
constexpr long long kQLimit = (1LL << 29) - 1;

// what a resampling pass reads: filled by pf_decide_kernel (an update) or pf_scan_sums_kernel (slam_pf_resample_indices_dev)
struct ScanHead {
    unsigned long long W, r;
    int                go, pad;
};

// the state record (device): the counter, the last update's sums and flags
struct State {
    unsigned long long amax_key; // (uint64)A_max ^ 2^63: unsigned order = signed order; 0 = no finite particle yet
    unsigned long long W, S2;
    long long          MX, MY, MC, MS;
    long long          n_resamples;
    unsigned           t;
    int                best, resampled, degenerate, refused, pad;
    ScanHead           head, dbg;
};

using Motion = slam_pf_motion; // as the device reads it
using Params = slam_pf_params;

struct Tables {
    const double   *cs, *G;
    const uint32_t *wtab;
    int             A, bits, L, shift;
};

struct Particles {
    double    *x, *y;
    int32_t   *k;
    long long *acc;
};

__device__ inline void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4])
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

__global__ __launch_bounds__(kBlock) void pf_words_kernel(unsigned p0, int n, unsigned t, unsigned purpose, unsigned k0, unsigned k1, uint32_t *words)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    unsigned w[4];
    philox4x32_10(p0 + (unsigned)i, t, purpose, 0u, k0, k1, w);
    for (int j = 0; j < 4; ++j) words[4 * (size_t)i + j] = w[j];
}

__device__ inline bool motion_ok(const Motion &m)
{
    return isfinite(m.dx) && isfinite(m.dy) && isfinite(m.sx) && isfinite(m.sy) && isfinite(m.sk) && m.sx >= 0.0 && m.sy >= 0.0 && m.sk >= 0.0 &&
           m.sk < kStepLimit && m.dk > -(1 << 20) && m.dk < (1 << 20);
}

// one draw of the motion model about (x, y, k): docs/PARTICLE_FILTER.md section 4
__device__ inline void draw(const Tables &T, const Motion &m, const unsigned w[4], double &x, double &y, int &k)
{
    const int    sh = 32 - T.bits;
    const double g0 = T.G[w[0] >> sh], g1 = T.G[w[1] >> sh], g2 = T.G[w[2] >> sh];
    const double c = T.cs[2 * k], s = T.cs[2 * k + 1];
    const double ex = __dadd_rn(m.dx, __dmul_rn(m.sx, g0)), ey = __dadd_rn(m.dy, __dmul_rn(m.sy, g1));
    x = __dadd_rn(x, __dsub_rn(__dmul_rn(c, ex), __dmul_rn(s, ey)));
    y = __dadd_rn(y, __dadd_rn(__dmul_rn(s, ex), __dmul_rn(c, ey)));
    k = (k + m.dk + (int)rint(__dmul_rn(m.sk, g2))) & (T.A - 1); // |sk g| < 2^20 * 2^10 (set_tables bounds G): the sum stays an int; A is a power of two
}

// init = false: predict (purpose 0, the particle's own pose); init = true: slam_pf_init_gaussian (purpose 1, every particle from
// the one pose (x0, y0, k0i), acc = 0)
__global__ __launch_bounds__(kBlock) void pf_predict_kernel(Tables T, Particles P, int n, const State *state, const Motion *motion, bool init,
                                                            double x0, double y0, int k0i, unsigned key0, unsigned key1)
{
    const Motion m = *motion;
    if (!motion_ok(m)) return; // uniform over the launch: pf_advance_kernel counts it
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    unsigned w[4];
    philox4x32_10((unsigned)p, state->t, init ? 1u : 0u, 0u, key0, key1, w);
    double x = init ? x0 : P.x[p], y = init ? y0 : P.y[p];
    int    k = init ? k0i : P.k[p];
    draw(T, m, w, x, y, k);
    P.x[p] = x, P.y[p] = y, P.k[p] = k;
    if (init) P.acc[p] = 0;
}

__global__ void pf_advance_kernel(State *state, const Motion *motion)
{
    if (motion_ok(*motion))
        state->t += 1u;
    else
        state->refused += 1;
}

// ------------------------------------------------------------------------------------------------------------ the update
__global__ __launch_bounds__(kBlock) void pf_poses_kernel(Tables T, Particles P, int n, double cx, double cy, double *poses, State *state)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p == 0) { // the sums of this update start from nothing; the launches that add to them come later on the stream
        state->amax_key = 0, state->W = 0, state->S2 = 0, state->MX = 0, state->MY = 0, state->MC = 0, state->MS = 0;
        state->best = 0x7fffffff, state->resampled = 0, state->degenerate = 0;
        state->head.W = 0, state->head.r = 0, state->head.go = 0;
    }
    if (p >= n) return;
    const int k = P.k[p];
    poses[4 * (size_t)p] = T.cs[2 * k], poses[4 * (size_t)p + 1] = T.cs[2 * k + 1];
    poses[4 * (size_t)p + 2] = __dsub_rn(P.x[p], cx), poses[4 * (size_t)p + 3] = __dsub_rn(P.y[p], cy);
}

__device__ inline unsigned long long shfl_down64(unsigned long long v, int d)
{
    const unsigned lo = __shfl_down((unsigned)v, d), hi = __shfl_down((unsigned)(v >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}

// the block's sum (wrapping, so two's-complement sums go through it as well) in thread 0; red: kBlock / 64 words
__device__ inline unsigned long long block_sum(unsigned long long v, unsigned long long *red)
{
    for (int d = 32; d; d >>= 1) v += shfl_down64(v, d);
    __syncthreads(); // red may still be read by the call before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < kBlock / 64; ++i) v += red[i];
    return v;
}

__device__ inline unsigned long long block_max(unsigned long long v, unsigned long long *red)
{
    for (int d = 32; d; d >>= 1) {
        const unsigned long long o = shfl_down64(v, d);
        v = o > v ? o : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < kBlock / 64; ++i) v = red[i] > v ? red[i] : v;
    return v;
}

__device__ inline bool finite_particle(const Particles &P, int p) { return isfinite(P.x[p]) && isfinite(P.y[p]); }

__global__ __launch_bounds__(kBlock) void pf_accumulate_kernel(Particles P, int n, const int32_t *score, State *state)
{
    __shared__ unsigned long long red[kBlock / 64];
    const int          p = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long key = 0; // below every real key: a real acc never reaches -2^63
    if (p < n) {
        const long long a = P.acc[p] + (long long)score[p];
        P.acc[p] = a;
        if (finite_particle(P, p)) key = (unsigned long long)a ^ 0x8000000000000000ull;
    }
    key = block_max(key, red);
    if (threadIdx.x == 0 && key) atomicMax(&state->amax_key, key);
}

// the inclusive scan of one block's kBlock values, in place in `buf` (2 kBlock words: two halves that take turns)
__device__ inline unsigned long long block_scan(unsigned long long v, unsigned long long *buf)
{
    int cur = 0;
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
        unsigned long long s = buf[cur * kBlock + threadIdx.x];
        if ((int)threadIdx.x >= d) s += buf[cur * kBlock + threadIdx.x - d];
        cur ^= 1;
        buf[cur * kBlock + threadIdx.x] = s;
        __syncthreads();
    }
    return buf[cur * kBlock + threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void pf_weights_kernel(Tables T, Particles P, int n, State *state, uint32_t *w_out, unsigned long long *C,
                                                            unsigned long long *sums)
{
    __shared__ unsigned long long buf[2 * kBlock];
    __shared__ unsigned long long red[kBlock / 64];
    const int                p = blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long amax_key = state->amax_key;
    unsigned long long       w = 0;
    long long                qx = 0, qy = 0, qc = 0, qs = 0;
    if (p < n && amax_key && finite_particle(P, p)) {
        const long long          amax = (long long)(amax_key ^ 0x8000000000000000ull), a = P.acc[p];
        const unsigned long long d = (unsigned long long)(amax - a) >> T.shift;
        w = T.wtab[d < (unsigned long long)(T.L - 1) ? (int)d : T.L - 1];
        if (a == amax) atomicMin(&state->best, p);
        const double sx = __dmul_rn(P.x[p], 65536.0), sy = __dmul_rn(P.y[p], 65536.0);
        qx = sx >= (double)kQLimit ? kQLimit : (sx <= -(double)kQLimit ? -kQLimit : __double2ll_rn(sx));
        qy = sy >= (double)kQLimit ? kQLimit : (sy <= -(double)kQLimit ? -kQLimit : __double2ll_rn(sy));
        const int k = P.k[p];
        qc = __double2ll_rn(__dmul_rn(T.cs[2 * k], 16777216.0)), qs = __double2ll_rn(__dmul_rn(T.cs[2 * k + 1], 16777216.0));
    }
    if (p < n) w_out[p] = (uint32_t)w;
    const unsigned long long c = block_scan(w, buf);
    if (p < n) C[p] = c;
    if (threadIdx.x == kBlock - 1) sums[blockIdx.x] = c;
    const unsigned long long sW = block_sum(w, red), sS2 = block_sum(w * w, red);
    const unsigned long long sX = block_sum(w * (unsigned long long)qx, red), sY = block_sum(w * (unsigned long long)qy, red);
    const unsigned long long sC = block_sum(w * (unsigned long long)qc, red), sS = block_sum(w * (unsigned long long)qs, red);
    if (threadIdx.x == 0 && sW) { // a block without weight adds nothing
        atomicAdd(&state->W, sW), atomicAdd(&state->S2, sS2);
        atomicAdd((unsigned long long *)&state->MX, sX), atomicAdd((unsigned long long *)&state->MY, sY);
        atomicAdd((unsigned long long *)&state->MC, sC), atomicAdd((unsigned long long *)&state->MS, sS);
    }
}

// the scan blocks of weights given from outside (slam_pf_resample_indices_dev)
__global__ __launch_bounds__(kBlock) void pf_scan_blocks_kernel(const uint32_t *w_in, int n, unsigned long long *C, unsigned long long *sums)
{
    __shared__ unsigned long long buf[2 * kBlock];
    const int          p = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long w = 0;
    if (p < n) w = w_in[p] > kPfWeightOne ? kPfWeightOne : w_in[p];
    const unsigned long long c = block_scan(w, buf);
    if (p < n) C[p] = c;
    if (threadIdx.x == kBlock - 1) sums[blockIdx.x] = c;
}

// One workgroup: sums[b] becomes the sum of the blocks before b (kBlock at a time with a carry, in place), and the total is returned
// to every thread.
__device__ inline unsigned long long scan_sums(unsigned long long *sums, int nb, unsigned long long *buf)
{
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += kBlock) {
        const int                b = base + threadIdx.x;
        const unsigned long long v = b < nb ? sums[b] : 0;
        const unsigned long long c = block_scan(v, buf), before = carry;
        if (b < nb) sums[b] = before + c - v;
        __syncthreads(); // everyone has read carry and buf
        if (threadIdx.x == kBlock - 1) carry = before + c;
        __syncthreads();
    }
    return carry;
}

// One workgroup after the weights: the decision (thread 0) and the scan of the block sums.
__global__ __launch_bounds__(kBlock) void pf_decide_kernel(State *state, int n, int num, int den, unsigned key0, unsigned key1, unsigned long long *sums,
                                                           int nb)
{
    __shared__ unsigned long long buf[2 * kBlock];
    const unsigned long long total = scan_sums(sums, nb, buf);
    if (threadIdx.x != 0) return;
    const unsigned long long W = state->W, S2 = state->S2;
    if (W == 0) { // no finite particle
        state->degenerate = 1, state->best = -1;
        return;
    }
    const unsigned __int128 lhs = (unsigned __int128)W * W * (unsigned)den, rhs = (unsigned __int128)S2 * (unsigned)n * (unsigned)num;
    if (!(lhs < rhs)) return;
    unsigned w[4];
    philox4x32_10(0u, state->t, 2u, 0u, key0, key1, w);
    state->resampled = 1, state->n_resamples += 1;
    state->head.W = total, state->head.r = (((unsigned long long)w[0] << 32) | w[1]) % total, state->head.go = 1; // total == W
}

__global__ __launch_bounds__(kBlock) void pf_scan_sums_kernel(ScanHead *head, unsigned long long r, unsigned long long *sums, int nb)
{
    __shared__ unsigned long long buf[2 * kBlock];
    const unsigned long long total = scan_sums(sums, nb, buf);
    if (threadIdx.x == 0) head->W = total, head->r = total ? r % total : 0, head->go = 1;
}

// src(j) = min { i : C_i n > j W + r }: C_i = sums[i / kBlock] + C[i] never falls, and C_(n-1) n = W n > j W + r.  With src, the
// index is written; with P2, particle src(j) is gathered into the second buffer.
__global__ __launch_bounds__(kBlock) void pf_search_kernel(const ScanHead *head, const unsigned long long *C, const unsigned long long *sums, int n,
                                                           int32_t *src, Particles P, Particles P2)
{
    if (!head->go) return;
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const unsigned long long W = head->W;
    int                      lo = j;
    if (W) {
        const unsigned long long target = (unsigned long long)j * W + head->r;
        int                      hi = n - 1;
        lo = 0;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((sums[mid / kBlock] + C[mid]) * (unsigned long long)n > target)
                hi = mid;
            else
                lo = mid + 1;
        }
    }
    if (src) src[j] = lo;
    if (P2.x) P2.x[j] = P.x[lo], P2.y[j] = P.y[lo], P2.k[j] = P.k[lo];
}

__global__ __launch_bounds__(kBlock) void pf_copy_back_kernel(const ScanHead *head, Particles P, Particles P2, int n)
{
    if (!head->go) return;
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    P.x[j] = P2.x[j], P.y[j] = P2.y[j], P.k[j] = P2.k[j], P.acc[j] = 0;
}

inline unsigned blocks_of(int n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int check_params(const Params &p)
{
    SLAM_REQUIRE(p.n_particles >= 1 && p.n_particles <= kMaxParticles, SLAM_E_INVALID, "slam_pf_create: n_particles %d is not in 1 .. 2^18",
                 p.n_particles);
    SLAM_REQUIRE(p.n_angles >= kPfMinAngles && p.n_angles <= kPfMaxAngles && !(p.n_angles & (p.n_angles - 1)), SLAM_E_INVALID,
                 "slam_pf_create: n_angles %d is not a power of two from 2^6 to 2^16", p.n_angles);
    SLAM_REQUIRE(p.gauss_bits >= kPfMinGaussBits && p.gauss_bits <= kPfMaxGaussBits, SLAM_E_INVALID, "slam_pf_create: gauss_bits %d is not in 4 .. 16",
                 p.gauss_bits);
    SLAM_REQUIRE(p.weight_len >= 2 && p.weight_len <= kPfMaxWeightLen, SLAM_E_INVALID, "slam_pf_create: weight_len %d is not in 2 .. 65536",
                 p.weight_len);
    SLAM_REQUIRE(p.weight_shift >= 0 && p.weight_shift <= kPfMaxWeightShift, SLAM_E_INVALID, "slam_pf_create: weight_shift %d is not in 0 .. 14",
                 p.weight_shift);
    SLAM_REQUIRE(std::isfinite(p.weight_scale) && p.weight_scale > 0.0, SLAM_E_INVALID, "slam_pf_create: weight_scale must be positive and finite");
    SLAM_REQUIRE(p.resample_num >= 0 && p.resample_num <= 65535 && p.resample_den >= 1 && p.resample_den <= 65535, SLAM_E_INVALID,
                 "slam_pf_create: resample_num / resample_den %d / %d: 0 .. 65535 over 1 .. 65535", p.resample_num, p.resample_den);
    return SLAM_OK;
}

const char *motion_refusal(const Motion &m)
{
    if (!std::isfinite(m.dx) || !std::isfinite(m.dy)) return "a non-finite increment";
    if (!std::isfinite(m.sx) || !std::isfinite(m.sy) || !std::isfinite(m.sk)) return "a non-finite sigma";
    if (m.sx < 0.0 || m.sy < 0.0 || m.sk < 0.0) return "a negative sigma";
    if (m.sk >= kStepLimit) return "sk at or beyond 2^20 heading steps";
    if (m.dk <= -(1 << 20) || m.dk >= (1 << 20)) return "|dk| at or beyond 2^20 heading steps";
    return nullptr;
}

} // namespace

struct slam_pf {
    Params P;
    DevMem         x, y, k, acc, x2, y2, k2; // the particles and the buffer a resample gathers into
    DevMem         cs, G, wtab;              // the tables
    DevMem         state, motion;            // the state record; the host forms' motion
    DevMem         poses, score, w, C, sums; // scratch of an update: 4 n f64, 2 n int32, n u32, n u64, n / kBlock u64
    DevMem         pts;                      // staging of slam_pf_update

    int       n() const { return P.n_particles; }
    unsigned  key0() const { return (unsigned)P.seed; }
    unsigned  key1() const { return (unsigned)(P.seed >> 32); }
    State    *st() const { return state.as<State>(); }
    Tables    tables() const { return Tables{cs.as<double>(), G.as<double>(), wtab.as<uint32_t>(), P.n_angles, P.gauss_bits, P.weight_len, P.weight_shift}; }
    Particles particles() const { return Particles{x.as<double>(), y.as<double>(), k.as<int32_t>(), acc.as<long long>()}; }
    Particles second() const { return Particles{x2.as<double>(), y2.as<double>(), k2.as<int32_t>(), nullptr}; }
};

extern "C" {

void slam_pf_default_params(slam_pf_params *p)
{
    if (!p) return;
    p->n_particles = 1024, p->n_angles = 4096, p->gauss_bits = 12;
    p->weight_len = 1024, p->weight_shift = 4, p->weight_scale = 1024.0;
    p->resample_num = 1, p->resample_den = 2, p->seed = 1;
}

int slam_pf_angle_table(int n_angles, double *cs, int n)
{
    const char *why;
    if (pf_angle_table(n_angles, cs, n, &why) != 0) {
        set_error("slam_pf_angle_table: %s", why);
        return SLAM_E_INVALID;
    }
    return SLAM_OK;
}

int slam_pf_gauss_table(int bits, double *G, int n)
{
    const char *why;
    if (pf_gauss_table(bits, G, n, &why) != 0) {
        set_error("slam_pf_gauss_table: %s", why);
        return SLAM_E_INVALID;
    }
    return SLAM_OK;
}

int slam_pf_weight_table(double scale, int shift, int L, uint32_t *wtab)
{
    const char *why;
    if (pf_weight_table(scale, shift, L, wtab, &why) != 0) {
        set_error("slam_pf_weight_table: %s", why);
        return SLAM_E_INVALID;
    }
    return SLAM_OK;
}

int slam_pf_set_tables(slam_pf_t *pf, const double *cs, int n_cs, const double *G, int n_G, const uint32_t *wtab, int n_w)
{
    SLAM_REQUIRE(pf, SLAM_E_INVALID, "slam_pf_set_tables: null handle");
    if (cs) {
        SLAM_REQUIRE(n_cs == 2 * pf->P.n_angles, SLAM_E_INVALID, "slam_pf_set_tables: the angle table has %d entries, not %d", 2 * pf->P.n_angles, n_cs);
        for (int i = 0; i < n_cs; ++i) SLAM_REQUIRE(std::isfinite(cs[i]), SLAM_E_INVALID, "slam_pf_set_tables: angle entry %d is not finite", i);
    }
    if (G) {
        SLAM_REQUIRE(n_G == 1 << pf->P.gauss_bits, SLAM_E_INVALID, "slam_pf_set_tables: the Gaussian table has %d entries, not %d",
                     1 << pf->P.gauss_bits, n_G);
        for (int i = 0; i < n_G; ++i)
            SLAM_REQUIRE(std::isfinite(G[i]) && std::fabs(G[i]) <= 1024.0, SLAM_E_INVALID, "slam_pf_set_tables: Gaussian entry %d is not within +-1024", i);
    }
    if (wtab) {
        SLAM_REQUIRE(n_w == pf->P.weight_len, SLAM_E_INVALID, "slam_pf_set_tables: the weight table has %d entries, not %d", pf->P.weight_len, n_w);
        SLAM_REQUIRE(pf_weight_table_ok(wtab, n_w), SLAM_E_INVALID, "slam_pf_set_tables: wtab[0] must be 65536 and no entry above it");
    }
    if (cs) SLAM_HIP(hipMemcpy(pf->cs.p, cs, sizeof(double) * (size_t)n_cs, hipMemcpyHostToDevice));
    if (G) SLAM_HIP(hipMemcpy(pf->G.p, G, sizeof(double) * (size_t)n_G, hipMemcpyHostToDevice));
    if (wtab) SLAM_HIP(hipMemcpy(pf->wtab.p, wtab, sizeof(uint32_t) * (size_t)n_w, hipMemcpyHostToDevice));
    return SLAM_OK;
}

static int create_filled(slam_pf *s)
{
    const Params &p = s->P;
    const size_t          n = (size_t)p.n_particles, nb = blocks_of(p.n_particles);
    SLAM_TRY(s->x.alloc(sizeof(double) * n));
    SLAM_TRY(s->y.alloc(sizeof(double) * n));
    SLAM_TRY(s->k.alloc(sizeof(int32_t) * n));
    SLAM_TRY(s->acc.alloc(sizeof(long long) * n));
    SLAM_TRY(s->x2.alloc(sizeof(double) * n));
    SLAM_TRY(s->y2.alloc(sizeof(double) * n));
    SLAM_TRY(s->k2.alloc(sizeof(int32_t) * n));
    SLAM_TRY(s->cs.alloc(sizeof(double) * 2 * (size_t)p.n_angles));
    SLAM_TRY(s->G.alloc(sizeof(double) << p.gauss_bits));
    SLAM_TRY(s->wtab.alloc(sizeof(uint32_t) * (size_t)p.weight_len));
    SLAM_TRY(s->state.alloc(sizeof(State)));
    SLAM_TRY(s->motion.alloc(sizeof(Motion)));
    SLAM_TRY(s->poses.alloc(sizeof(double) * 4 * n));
    SLAM_TRY(s->score.alloc(sizeof(int32_t) * 2 * n));
    SLAM_TRY(s->w.alloc(sizeof(uint32_t) * n));
    SLAM_TRY(s->C.alloc(sizeof(unsigned long long) * n));
    SLAM_TRY(s->sums.alloc(sizeof(unsigned long long) * nb));
    for (DevMem *m : {&s->x, &s->y, &s->k, &s->acc, &s->x2, &s->y2, &s->k2, &s->state, &s->motion, &s->w, &s->C, &s->sums})
        SLAM_HIP(hipMemset(m->p, 0, m->cap));
    std::vector<double>   cs(2 * (size_t)p.n_angles), G((size_t)1 << p.gauss_bits);
    std::vector<uint32_t> wtab((size_t)p.weight_len);
    const char           *why = "";
    if (pf_angle_table(p.n_angles, cs.data(), (int)cs.size(), &why) != 0 || pf_gauss_table(p.gauss_bits, G.data(), (int)G.size(), &why) != 0 ||
        pf_weight_table(p.weight_scale, p.weight_shift, p.weight_len, wtab.data(), &why) != 0) {
        set_error("slam_pf_create: %s", why);
        return SLAM_E_INVALID;
    }
    return slam_pf_set_tables(s, cs.data(), (int)cs.size(), G.data(), (int)G.size(), wtab.data(), (int)wtab.size());
}

int slam_pf_create(const slam_pf_params *params, slam_pf_t **out)
{
    SLAM_REQUIRE(out, SLAM_E_INVALID, "slam_pf_create: null out pointer");
    *out = nullptr;
    Params p;
    slam_pf_default_params(&p);
    if (params) p = *params;
    SLAM_TRY(check_params(p));
    SLAM_TRY(require_device());
    slam_pf *s = new (std::nothrow) slam_pf();
    SLAM_REQUIRE(s, SLAM_E_NOMEM, "slam_pf_create: out of host memory");
    s->P = p;
    const int rc = create_filled(s);
    if (rc != SLAM_OK) {
        delete s;
        return rc;
    }
    *out = s;
    return SLAM_OK;
}

void slam_pf_destroy(slam_pf_t *pf)
{
    delete pf; // (hipFree waits for what is still enqueued)
}

int slam_pf_set_particles(slam_pf_t *pf, const double *x, const double *y, const int32_t *k, int n)
{
    SLAM_REQUIRE(pf && x && y && k, SLAM_E_INVALID, "slam_pf_set_particles: null argument");
    SLAM_REQUIRE(n == pf->n(), SLAM_E_INVALID, "slam_pf_set_particles: %d particles given, the filter has %d", n, pf->n());
    for (int i = 0; i < n; ++i)
        SLAM_REQUIRE(k[i] >= 0 && k[i] < pf->P.n_angles, SLAM_E_INVALID, "slam_pf_set_particles: heading %d of particle %d is not in [0, %d)", k[i], i,
                     pf->P.n_angles);
    SLAM_HIP(hipMemcpy(pf->x.p, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    SLAM_HIP(hipMemcpy(pf->y.p, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    SLAM_HIP(hipMemcpy(pf->k.p, k, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    SLAM_HIP(hipMemset(pf->acc.p, 0, sizeof(long long) * (size_t)n));
    return SLAM_OK;
}

int slam_pf_read_particles(slam_pf_t *pf, double *x, double *y, int32_t *k)
{
    SLAM_REQUIRE(pf, SLAM_E_INVALID, "slam_pf_read_particles: null handle");
    const size_t n = (size_t)pf->n();
    if (x) SLAM_HIP(hipMemcpy(x, pf->x.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (y) SLAM_HIP(hipMemcpy(y, pf->y.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (k) SLAM_HIP(hipMemcpy(k, pf->k.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    if (!x && !y && !k) SLAM_HIP(hipDeviceSynchronize());
    return SLAM_OK;
}

int slam_pf_read_weights(slam_pf_t *pf, int64_t *acc, uint32_t *w)
{
    SLAM_REQUIRE(pf, SLAM_E_INVALID, "slam_pf_read_weights: null handle");
    const size_t n = (size_t)pf->n();
    if (acc) SLAM_HIP(hipMemcpy(acc, pf->acc.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    if (w) SLAM_HIP(hipMemcpy(w, pf->w.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_pf_read_state(slam_pf_t *pf, slam_pf_state *out)
{
    SLAM_REQUIRE(pf && out, SLAM_E_INVALID, "slam_pf_read_state: null argument");
    State s;
    SLAM_HIP(hipDeviceSynchronize()); // whatever stream the last update ran on
    SLAM_HIP(hipMemcpy(&s, pf->state.p, sizeof(State), hipMemcpyDeviceToHost));
    out->t = (int64_t)s.t, out->n = pf->n(), out->resampled = s.resampled, out->degenerate = s.degenerate;
    out->best = s.W ? s.best : -1, out->refused = s.refused, out->n_resamples = s.n_resamples;
    out->A_max = s.W ? (int64_t)(s.amax_key ^ 0x8000000000000000ull) : 0;
    out->W = (int64_t)s.W, out->S2 = (int64_t)s.S2, out->MX = s.MX, out->MY = s.MY, out->MC = s.MC, out->MS = s.MS;
    if (s.W) {
        const double den = (double)s.W * 65536.0;
        out->x = (double)s.MX / den, out->y = (double)s.MY / den, out->theta = std::atan2((double)s.MS, (double)s.MC);
    } else {
        out->x = out->y = out->theta = std::nan("");
    }
    return SLAM_OK;
}

int slam_pf_random_words_dev(slam_pf_t *pf, uint32_t p0, int n, uint32_t t, uint32_t purpose, uint32_t *d_words)
{
    SLAM_REQUIRE(pf && n >= 0 && n <= kMaxWords, SLAM_E_INVALID, "slam_pf_random_words_dev: bad arguments (at most 2^20 counters)");
    if (n == 0) return SLAM_OK;
    SLAM_REQUIRE(d_words, SLAM_E_INVALID, "slam_pf_random_words_dev: null array");
    hipLaunchKernelGGL(pf_words_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, nullptr, p0, n, t, purpose, pf->key0(), pf->key1(), d_words);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

static int predict_launch(slam_pf_t *pf, const Motion *d_motion, bool init, double x0, double y0, int k0, hipStream_t st)
{
    hipLaunchKernelGGL(pf_predict_kernel, dim3(blocks_of(pf->n())), dim3(kBlock), 0, st, pf->tables(), pf->particles(), pf->n(), pf->st(), d_motion, init,
                       x0, y0, k0, pf->key0(), pf->key1());
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int slam_pf_predict_dev(slam_pf_t *pf, const slam_pf_motion *d_motion, slam_stream_t stream)
{
    SLAM_REQUIRE(pf && d_motion, SLAM_E_INVALID, "slam_pf_predict_dev: null argument");
    SLAM_TRY(predict_launch(pf, d_motion, false, 0.0, 0.0, 0, as_stream(stream)));
    hipLaunchKernelGGL(pf_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), pf->st(), d_motion);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int slam_pf_predict(slam_pf_t *pf, const slam_pf_motion *motion)
{
    SLAM_REQUIRE(pf, SLAM_E_INVALID, "slam_pf_predict: null handle");
    SLAM_REQUIRE(motion, SLAM_E_INVALID, "slam_pf_predict: null motion");
    const char *why = motion_refusal(*motion);
    SLAM_REQUIRE(!why, SLAM_E_INVALID, "slam_pf_predict: %s", why);
    SLAM_HIP(hipMemcpy(pf->motion.p, motion, sizeof(Motion), hipMemcpyHostToDevice));
    SLAM_TRY(slam_pf_predict_dev(pf, pf->motion.as<Motion>(), nullptr));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

int slam_pf_init_gaussian(slam_pf_t *pf, double x, double y, int k, double sx, double sy, double sk)
{
    SLAM_REQUIRE(pf, SLAM_E_INVALID, "slam_pf_init_gaussian: null handle");
    SLAM_REQUIRE(std::isfinite(x) && std::isfinite(y) && k >= 0 && k < pf->P.n_angles, SLAM_E_INVALID,
                 "slam_pf_init_gaussian: the pose must be finite with its heading in [0, %d)", pf->P.n_angles);
    const Motion m = {0.0, 0.0, sx, sy, sk, 0, 0};
    const char          *why = motion_refusal(m);
    SLAM_REQUIRE(!why, SLAM_E_INVALID, "slam_pf_init_gaussian: %s", why);
    SLAM_HIP(hipMemcpy(pf->motion.p, &m, sizeof(m), hipMemcpyHostToDevice));
    SLAM_TRY(predict_launch(pf, pf->motion.as<Motion>(), true, x, y, k, nullptr));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

int slam_pf_update_dev(slam_pf_t *pf, slam_csm_t *csm, const double *d_pts, int n, int n_ga, double cx, double cy, slam_stream_t stream)
{
    SLAM_REQUIRE(pf && csm, SLAM_E_INVALID, "slam_pf_update_dev: null handle");
    SLAM_REQUIRE(n >= 0 && n <= (1 << 23) && (n == 0 || d_pts), SLAM_E_INVALID, "slam_pf_update_dev: bad scan (at most 2^23 points)");
    SLAM_REQUIRE(std::isfinite(cx) && std::isfinite(cy), SLAM_E_INVALID, "slam_pf_update_dev: the window's centre is not finite");
    const hipStream_t st = as_stream(stream);
    const int         N = pf->n(), nb = (int)blocks_of(N);
    const dim3        grid(blocks_of(N)), block(kBlock);
    const Tables      T = pf->tables();
    const Particles   P = pf->particles(), P2 = pf->second();
    int32_t          *score = pf->score.as<int32_t>();
    auto             *C = pf->C.as<unsigned long long>(), *sums = pf->sums.as<unsigned long long>();
    hipLaunchKernelGGL(pf_poses_kernel, grid, block, 0, st, T, P, N, cx, cy, pf->poses.as<double>(), pf->st());
    SLAM_HIP(hipGetLastError());
    SLAM_TRY(slam_csm_score_poses_dev(csm, d_pts, n, n_ga, pf->poses.as<double>(), N, score, score + N, stream));
    hipLaunchKernelGGL(pf_accumulate_kernel, grid, block, 0, st, P, N, score, pf->st());
    hipLaunchKernelGGL(pf_weights_kernel, grid, block, 0, st, T, P, N, pf->st(), pf->w.as<uint32_t>(), C, sums);
    hipLaunchKernelGGL(pf_decide_kernel, dim3(1), block, 0, st, pf->st(), N, pf->P.resample_num, pf->P.resample_den, pf->key0(), pf->key1(), sums, nb);
    hipLaunchKernelGGL(pf_search_kernel, grid, block, 0, st, &pf->st()->head, C, sums, N, (int32_t *)nullptr, P, P2);
    hipLaunchKernelGGL(pf_copy_back_kernel, grid, block, 0, st, &pf->st()->head, P, P2, N);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int slam_pf_update(slam_pf_t *pf, slam_csm_t *csm, const double *pts, int n, int n_ga, double cx, double cy)
{
    SLAM_REQUIRE(pf && csm, SLAM_E_INVALID, "slam_pf_update: null handle");
    SLAM_REQUIRE(n >= 0 && n <= (1 << 23) && (n == 0 || pts), SLAM_E_INVALID, "slam_pf_update: bad scan (at most 2^23 points)");
    SLAM_REQUIRE(std::isfinite(cx) && std::isfinite(cy), SLAM_E_INVALID, "slam_pf_update: the window's centre is not finite");
    const size_t bytes = sizeof(double) * 2 * (size_t)n;
    SLAM_TRY(reserve_quarter(pf->pts, bytes));
    if (n) SLAM_HIP(hipMemcpyAsync(pf->pts.p, pts, bytes, hipMemcpyHostToDevice, nullptr));
    SLAM_TRY(slam_pf_update_dev(pf, csm, pf->pts.as<double>(), n, n_ga, cx, cy, nullptr));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

int slam_pf_resample_indices_dev(slam_pf_t *pf, const uint32_t *d_w, int n, uint64_t r, int32_t *d_src, slam_stream_t stream)
{
    SLAM_REQUIRE(pf && d_w && d_src, SLAM_E_INVALID, "slam_pf_resample_indices_dev: null argument");
    SLAM_REQUIRE(n >= 1 && n <= pf->n(), SLAM_E_INVALID, "slam_pf_resample_indices_dev: %d weights, the filter has %d particles", n, pf->n());
    const hipStream_t st = as_stream(stream);
    const int         nb = (int)blocks_of(n);
    auto             *C = pf->C.as<unsigned long long>(), *sums = pf->sums.as<unsigned long long>();
    const Particles   none = {nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(pf_scan_blocks_kernel, dim3(nb), dim3(kBlock), 0, st, d_w, n, C, sums);
    hipLaunchKernelGGL(pf_scan_sums_kernel, dim3(1), dim3(kBlock), 0, st, &pf->st()->dbg, (unsigned long long)r, sums, nb);
    hipLaunchKernelGGL(pf_search_kernel, dim3(nb), dim3(kBlock), 0, st, &pf->st()->dbg, C, sums, n, d_src, none, none);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

} // extern "C"
