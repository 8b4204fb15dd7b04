// The scratch replacement of the batched tracker handle (iv_slam_amd/csrc/ivf_scratch.h) against a counting fake device, on the host:
// sets of 1, 2 and 9 buffers through first use, growth, a refused allocation at every position, a failing wait, and destroy after
// each.  Built with AddressSanitizer (leak check included) and UBSan by tests/test_scratch_cpu.py; exit 0 = every check held.
#include "ivf_scratch.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s (set of %d, k = %d)\n", __FILE__, __LINE__, #c, g_n, g_k); std::exit(1); } } while (0)
static int g_n = 0, g_k = 0;

struct FakeDevice {
    int failAt = 0;                         // the k-th allocation from now on is refused (1-based; 0: none)
    bool failWait = false;
    int allocs = 0, waits = 0, allocsAtWait = -1;
    std::vector<size_t> requests;           // bytes, in the order they arrived
    std::map<void*, int> freed;             // how often each pointer was given back
    std::vector<void*> live;

    void* alloc(size_t bytes)
    {
        requests.push_back(bytes);
        if (++allocs == failAt) return nullptr;
        void* p = std::malloc(bytes);
        live.push_back(p);
        return p;
    }
    void free(void* p)
    {
        if (freed[p]++ != 0) return;        // a second free is counted, not made
        CHECK(std::count(live.begin(), live.end(), p) == 1);
        live.erase(std::find(live.begin(), live.end(), p));
        std::free(p);
    }
    bool wait() { waits++; allocsAtWait = allocs; return !failWait; }
    void reset(int fail, bool fw) { failAt = fail; failWait = fw; allocs = waits = 0; allocsAtWait = -1; requests.clear(); freed.clear(); }
};

// a handle with nine slots of different pointee types, like the tracker's
struct Handle {
    int* a = nullptr; float* b = nullptr; unsigned short* c = nullptr; void* d = nullptr; double* e = nullptr;
    unsigned long long* f = nullptr; int* g = nullptr; unsigned* h = nullptr; char* i = nullptr;
    std::vector<void*> owned;
    void* at(int k) const { void* const v[9] = {a, b, c, d, e, f, g, h, i}; return v[k]; }
};

// sizes neither sorted nor all distinct: the order of the requests is the routine's doing
static const size_t kBytes[9] = {48, 512, 16, 512, 1024, 8, 96, 4, 256};

static bool replace(FakeDevice& dev, Handle& H, int n, size_t scale)
{
    const size_t* B = kBytes;
    if (n == 1) return ivf::scratch_replace(dev, H.owned, {{H.a, B[0] * scale}});
    if (n == 2) return ivf::scratch_replace(dev, H.owned, {{H.a, B[0] * scale}, {H.b, B[1] * scale}});
    return ivf::scratch_replace(dev, H.owned, {{H.a, B[0] * scale}, {H.b, B[1] * scale}, {H.c, B[2] * scale}, {H.d, B[3] * scale}, {H.e, B[4] * scale},
                                               {H.f, B[5] * scale}, {H.g, B[6] * scale}, {H.h, B[7] * scale}, {H.i, B[8] * scale}});
}

static std::vector<void*> slots_of(const Handle& H, int n)
{
    std::vector<void*> v;
    for (int k = 0; k < n; k++) v.push_back(H.at(k));
    return v;
}

static void check_descending(const FakeDevice& dev)
{
    for (size_t r = 1; r < dev.requests.size(); r++) CHECK(dev.requests[r - 1] >= dev.requests[r]);
}

// every slot of the set holds a live buffer, all distinct, and the ownership list names each of these slots exactly once
static void check_owned(const FakeDevice& dev, const Handle& H, int n)
{
    CHECK((int)H.owned.size() == n && (int)dev.live.size() == n);
    for (int k = 0; k < n; k++) {
        CHECK(H.at(k) != nullptr && std::count(dev.live.begin(), dev.live.end(), H.at(k)) == 1);
        for (int j = 0; j < k; j++) CHECK(H.at(j) != H.at(k));
    }
    const void* addr[9] = {&H.a, &H.b, &H.c, &H.d, &H.e, &H.f, &H.g, &H.h, &H.i};
    for (int k = 0; k < n; k++) CHECK(std::count(H.owned.begin(), H.owned.end(), addr[k]) == 1);
}

// after a refused growth: the slots hold their old pointers, none of which was freed; what was newly allocated was freed once; the list is as before
static void check_unchanged(const FakeDevice& dev, const Handle& H, int n, const std::vector<void*>& old, const std::vector<void*>& ownedBefore, int newAllocs)
{
    CHECK(slots_of(H, n) == old && H.owned == ownedBefore);
    for (void* p : old) CHECK(dev.freed.count(p) == 0);
    CHECK((int)dev.freed.size() == newAllocs);
    for (const auto& f : dev.freed) CHECK(f.second == 1);
    CHECK(dev.live.size() == old.size() - (size_t)std::count(old.begin(), old.end(), nullptr));
}

static void destroy(FakeDevice& dev, Handle& H, int n)
{
    const std::vector<void*> held = slots_of(H, n);
    dev.reset(0, false);
    ivf::scratch_free_all(dev, H.owned);
    for (void* p : held) CHECK(p == nullptr || dev.freed[p] == 1);
    CHECK(dev.live.empty() && H.owned.empty() && dev.freed.size() == held.size() - (size_t)std::count(held.begin(), held.end(), nullptr));
}

// a handle of n buffers after `grown` successful calls (1: first use only; 2: grown once)
static void build(FakeDevice& dev, Handle& H, int n, int grown)
{
    dev.reset(0, false);
    CHECK(replace(dev, H, n, 1));
    CHECK(dev.waits == 0 && dev.allocs == n);                          // first use: no wait
    check_descending(dev);
    check_owned(dev, H, n);
    if (grown < 2) return;
    const std::vector<void*> old = slots_of(H, n);
    dev.reset(0, false);
    CHECK(replace(dev, H, n, 3));
    CHECK(dev.waits == 1 && dev.allocsAtWait == n && dev.allocs == n); // growth: one wait, after every allocation
    check_descending(dev);
    for (void* p : old) CHECK(dev.freed[p] == 1);
    CHECK((int)dev.freed.size() == n);
    check_owned(dev, H, n);
    for (int k = 0; k < n; k++) CHECK(std::count(old.begin(), old.end(), H.at(k)) == 0);
}

int main()
{
    for (int n : {1, 2, 9}) {
        g_n = n;
        for (int grown : {1, 2}) {                                     // destroy after first use, after growth
            g_k = 0;
            FakeDevice dev; Handle H;
            build(dev, H, n, grown);
            destroy(dev, H, n);
        }
        for (int before : {0, 1, 2})                                   // a refusal at a first use, at a growth, at a second growth
            for (int k = 1; k <= n + 1; k++) {                         // k = n + 1: every allocation succeeds and the wait fails
                g_k = k;
                const bool waitFails = k == n + 1;
                if (waitFails && before == 0) continue;                // a first use does not wait
                FakeDevice dev; Handle H;
                if (before) build(dev, H, n, before);
                const std::vector<void*> old = slots_of(H, n), ownedBefore = H.owned;
                dev.reset(waitFails ? 0 : k, waitFails);
                CHECK(!replace(dev, H, n, 5));
                CHECK(dev.waits == (waitFails ? 1 : 0) && dev.allocs == (waitFails ? n : k));
                check_descending(dev);
                check_unchanged(dev, H, n, old, ownedBefore, waitFails ? n : k - 1);
                if (before) {                                          // the handle is as usable as before: it grows when there is room again
                    dev.reset(0, false);
                    CHECK(replace(dev, H, n, 5) && dev.waits == 1);
                    check_owned(dev, H, n);
                }
                destroy(dev, H, n);
            }
    }
    std::puts("scratch_host: ok");
    return 0;
}
