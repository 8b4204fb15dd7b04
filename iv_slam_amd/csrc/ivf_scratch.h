// ivf_scratch.h -- the one statement of how the batched tracker handle (ivf_tracker.h) allocates, grows and gives back its device scratch.
// Host-only C++17, no HIP header: the device is a policy type with void* alloc(size_t bytes) (null: refused), void free(void*) and bool
// wait() (for the handle's previous call; false: the wait itself failed), HIP's in ivf_tracker.h, a counting fake in tests/scratch/scratch_host.cpp.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
namespace ivf {
// one buffer of a set: the pointer object that names it, by its address (any pointee type: read and written as bytes), and the size it is to get
inline void* scratch_get(const void* slot) { void* p; std::memcpy(&p, slot, sizeof p); return p; }
inline void scratch_set(void* slot, void* p) { std::memcpy(slot, &p, sizeof p); }
struct ScratchSlot { void* slot; size_t bytes; template <class T> ScratchSlot(T*& p, size_t n) : slot(&p), bytes(n) {} };

// Replaces the buffers of `set` (all null: a first use) by new ones of the given sizes.  `owned` lists the slots that hold a buffer.
// Every new buffer is allocated first, the largest first, so that a hopeless request is refused before anything else is taken; then,
// only if there is an old buffer, the handle's previous call is waited for; then the old ones are freed and the slots set.  Old and new
// buffers are therefore live together until the swap: a growth needs room for both, and in return a failed allocation or wait gives the
// new ones back, leaves every slot, every old buffer and `owned` as they were, and returns false -- the handle stays usable with what it had.
template <class Device> bool scratch_replace(Device&& dev, std::vector<void*>& owned, std::initializer_list<ScratchSlot> set)
{
    std::vector<ScratchSlot> order(set);
    std::stable_sort(order.begin(), order.end(), [](const ScratchSlot& a, const ScratchSlot& b) { return a.bytes > b.bytes; });
    std::vector<void*> fresh;
    bool hadOld = false;
    for (const ScratchSlot& e : order) {
        hadOld = hadOld || scratch_get(e.slot);
        if (void* p = dev.alloc(e.bytes)) fresh.push_back(p); else break;
    }
    if (fresh.size() < order.size() || (hadOld && !dev.wait())) {
        for (void* p : fresh) dev.free(p);
        return false;
    }
    for (size_t i = 0; i < order.size(); i++) {
        if (void* old = scratch_get(order[i].slot)) dev.free(old);
        else owned.push_back(order[i].slot);                          // a slot is listed once, at its first buffer: it is never null again
        scratch_set(order[i].slot, fresh[i]);
    }
    return true;
}
// the end of the handle: every buffer it holds is given back (the slots keep their now stale pointers)
template <class Device> void scratch_free_all(Device&& dev, std::vector<void*>& owned)
{
    for (void* slot : owned) dev.free(scratch_get(slot));
    owned.clear();
}
}  // namespace ivf
