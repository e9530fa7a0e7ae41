// include/slam_amd/buffer.hpp on its own, under a host sanitizer: the six C-ABI functions it calls are stubs over malloc / free
// here that count live blocks and synchronise calls and can make the next allocation fail.  A stand-alone program:
//   g++ -std=c++17 -fsanitize=address,undefined adapter_buffer_test.cpp && ./a.out
// Exit 0 when every check holds and no block is left; the sanitizer's own exit status counts (tests/test_adapter_buffer.py).
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "slam_amd/buffer.hpp"

static std::set<void *> g_dev, g_pin; // live blocks
static int              g_sync = 0, g_frees = 0, g_fail_in = 0; // g_fail_in = k: the k-th allocation from now fails
static size_t           g_last_bytes = 0;
static int              g_events[64], g_n_events = 0; // 's' a synchronise, 'f' a free, in order

static void event(int e)
{
    if (g_n_events < 64) g_events[g_n_events++] = e;
}
static int stub_alloc(std::set<void *> &live, void **p, size_t bytes)
{
    *p = nullptr;
    if (g_fail_in > 0 && --g_fail_in == 0) return SLAM_E_NOMEM;
    *p = std::malloc(bytes ? bytes : 1);
    live.insert(*p);
    g_last_bytes = bytes;
    return SLAM_OK;
}
static int stub_free(std::set<void *> &live, void *p)
{
    if (!p) return SLAM_OK;
    if (!live.erase(p)) {
        std::fprintf(stderr, "freed a block that is not live (twice, or of the other kind)\n");
        std::abort();
    }
    std::free(p);
    ++g_frees;
    event('f');
    return SLAM_OK;
}
extern "C" {
int slam_malloc(void **p, size_t bytes) { return stub_alloc(g_dev, p, bytes); }
int slam_free(void *p) { return stub_free(g_dev, p); }
int slam_host_alloc(void **p, size_t bytes) { return stub_alloc(g_pin, p, bytes); }
int slam_host_free(void *p) { return stub_free(g_pin, p); }
int slam_device_synchronize(void)
{
    ++g_sync;
    event('s');
    return SLAM_OK;
}
const char *slam_last_error(void) { return "stub"; }
}

static int g_failed = 0;
#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #c); \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

using slam_amd::detail::DeviceBuffer;
using slam_amd::detail::PinnedBuffer;
static size_t live() { return g_dev.size() + g_pin.size(); }

template <class B>
static void one_kind(std::set<void *> &mine)
{
    {
        B b;
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.reserve(100) && b.cap == 100 && b.p && mine.size() == 1);
        // below the capacity: nothing happens
        void     *p = b.p;
        const int sync0 = g_sync, frees0 = g_frees;
        CHECK(b.reserve(100) && b.reserve(1) && b.reserve(0, 4000));
        CHECK(b.p == p && b.cap == 100 && g_sync == sync0 && g_frees == frees0);
        // growth: one synchronise, then one free, then max(need, alloc_bytes)
        g_n_events = 0;
        CHECK(b.reserve(101, 150) && b.cap == 150 && g_last_bytes == 150);
        CHECK(g_n_events == 2 && g_events[0] == 's' && g_events[1] == 'f' && mine.size() == 1);
        CHECK(b.reserve(400, 200) && b.cap == 400 && g_last_bytes == 400);
        CHECK(slam_amd::detail::reserve_quarter(b, 1000) && b.cap == 1250);
        CHECK(slam_amd::detail::reserve_half(b, 2000) && b.cap == 3000);
        CHECK(b.template as<int>() == static_cast<int *>(b.p));
        // a failed allocation: empty, and the next reserve starts clean
        g_fail_in = 1;
        CHECK(!b.reserve(5000) && b.p == nullptr && b.cap == 0 && mine.empty());
        g_n_events = 0;
        CHECK(b.reserve(10) && b.cap == 10 && g_n_events == 0 && mine.size() == 1); // (nothing held: nothing to wait for)
        g_fail_in = 1;
        CHECK(!b.alloc(20) && b.p == nullptr && b.cap == 0 && mine.empty());
        CHECK(b.alloc(20) && b.alloc(30) && b.cap == 30 && mine.size() == 1); // alloc gives back what it held
        b.release();
        CHECK(b.p == nullptr && b.cap == 0 && mine.empty());
        b.release();
        CHECK(b.alloc(8));
    } // the destructor frees
    CHECK(mine.empty());
    {
        B a, b;
        CHECK(a.alloc(16) && b.alloc(32));
        void *pa = a.p, *pb = b.p;
        B     c(std::move(a)); // move construction leaves the source empty
        CHECK(c.p == pa && c.cap == 16 && a.p == nullptr && a.cap == 0 && mine.size() == 2);
        b = std::move(c); // move assignment gives back what the target held
        CHECK(b.p == pa && b.cap == 16 && c.p == nullptr && c.cap == 0 && mine.size() == 1 && !mine.count(pb));
        B &self = b;
        b = std::move(self); // self-move: harmless
        CHECK(b.p == pa && b.cap == 16 && mine.size() == 1);
        CHECK(a.alloc(64));
        void *pa2 = a.p;
        std::swap(a, b);
        CHECK(a.p == pa && a.cap == 16 && b.p == pa2 && b.cap == 64 && mine.size() == 2);
    }
    CHECK(mine.empty());
}

// the shape of slam_amd::MLS::add_cloud: one capacity for four blocks, which grow together or not at all
static bool grow_four(DeviceBuffer (&b)[4], size_t &cap, size_t n)
{
    if (n <= cap) return true;
    cap = 0;
    if (!(b[0].reserve(32 * n) && b[1].reserve(n) && b[2].reserve(16 * n) && b[3].reserve(16 * n))) {
        for (DeviceBuffer &x : b) x.release();
        return false;
    }
    cap = n;
    return true;
}

int main()
{
    one_kind<DeviceBuffer>(g_dev);
    one_kind<PinnedBuffer>(g_pin);
    {
        DeviceBuffer four[4];
        size_t       cap = 0;
        CHECK(grow_four(four, cap, 100) && cap == 100 && g_dev.size() == 4);
        g_fail_in = 3; // the third of the four
        CHECK(!grow_four(four, cap, 200) && cap == 0 && g_dev.empty());
        for (const DeviceBuffer &x : four) CHECK(x.p == nullptr && x.cap == 0);
        CHECK(grow_four(four, cap, 50) && cap == 50 && g_dev.size() == 4); // the next call starts clean
    }
    {
        slam_amd::detail::Array<double> a; // reads as the pointer it replaces
        CHECK(a.alloc(4 * sizeof(double)));
        double *d = a;
        d[3] = 2.5;
        CHECK(a[3] == 2.5 && a + 1 == d + 1 && a.as<double>() == d);
    }
    slam_amd::detail::warn("adapter_buffer_test (expected line)");
    CHECK(live() == 0);
    if (g_failed) return 1;
    std::puts("ok");
    return 0;
}
