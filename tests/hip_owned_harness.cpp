// csrc/hip_owned.h on the CPU: the owners over counting stand-ins for the hip* calls they make (tests/test_hip_owned_cpu.py builds
// this with -fsanitize=address,undefined and runs it).  Every stand-in allocation is a malloc the sanitizer tracks, every handle
// is remembered in a set, and a release of something that is not in the set counts as a fault.
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <type_traits>
#include <utility>

typedef int hipError_t;
const hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
typedef struct ihipEvent_t *hipEvent_t;
typedef struct ihipStream_t *hipStream_t;

static std::set<void *> g_live;
static int g_allocs = 0, g_frees = 0, g_badFrees = 0;
static int g_failAfter = -1; // >= 0: the allocation after that many more fails

static hipError_t standInAlloc(void **p, size_t bytes)
{
    if (g_failAfter == 0)
    {
        g_failAfter = -1;
        *p = reinterpret_cast<void *>(0x1); // a failed call may leave anything in *p: the owner must not keep it
        return hipErrorOutOfMemory;
    }
    if (g_failAfter > 0)
        g_failAfter--;
    *p = malloc(bytes ? bytes : 1);
    g_live.insert(*p);
    g_allocs++;
    return hipSuccess;
}
static hipError_t standInFree(void *p)
{
    if (!g_live.erase(p))
    {
        g_badFrees++;
        return 1;
    }
    free(p);
    g_frees++;
    return hipSuccess;
}
static hipError_t hipMalloc(void **p, size_t bytes) { return standInAlloc(p, bytes); }
static hipError_t hipHostMalloc(void **p, size_t bytes) { return standInAlloc(p, bytes); }
static hipError_t hipFree(void *p) { return standInFree(p); }
static hipError_t hipHostFree(void *p) { return standInFree(p); }
static hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return standInAlloc(reinterpret_cast<void **>(e), 1); }
static hipError_t hipEventDestroy(hipEvent_t e) { return standInFree(e); }
static hipError_t hipStreamCreate(hipStream_t *s) { return standInAlloc(reinterpret_cast<void **>(s), 1); }
static hipError_t hipStreamDestroy(hipStream_t s) { return standInFree(s); }

#include "../convectionkernels_amd/csrc/hip_owned.h"

using namespace cvtt_owned;

// 4. the owners move and do not copy
static_assert(!std::is_copy_constructible<DeviceBuffer>::value && !std::is_copy_assignable<DeviceBuffer>::value, "DeviceBuffer copies");
static_assert(!std::is_copy_constructible<PinnedBuffer>::value && !std::is_copy_assignable<PinnedBuffer>::value, "PinnedBuffer copies");
static_assert(!std::is_copy_constructible<Event>::value && !std::is_copy_assignable<Event>::value, "Event copies");
static_assert(!std::is_copy_constructible<Stream>::value && !std::is_copy_assignable<Stream>::value, "Stream copies");
static_assert(std::is_nothrow_move_constructible<DeviceBuffer>::value && std::is_nothrow_move_assignable<Event>::value &&
              std::is_nothrow_move_constructible<Stream>::value, "the owners move");

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); g_failed++; } } while (0)

// a struct of owners, as the context is one
namespace
{
struct Slot
{
    PinnedBuffer pinnedIn, pinnedOut;
    DeviceBuffer dIn, dOut;
    Stream stream;
    Event done;
};
}

static bool balanced() { return g_live.empty() && g_allocs == g_frees && g_badFrees == 0; }

int main()
{
    // 1. every allocation is freed exactly once after moves, regrowth and scope exit
    {
        DeviceBuffer a;
        CHECK(!a && a.get() == NULL && a.bytes() == 0);
        CHECK(a.reserve(100) == hipSuccess && a && a.bytes() == 100 && g_allocs == 1);
        void *first = a.get();
        DeviceBuffer b(std::move(a));
        CHECK(!a && a.bytes() == 0 && b.get() == first && b.bytes() == 100 && g_frees == 0);
        CHECK(b.reserve(200) == hipSuccess && b.bytes() == 200 && g_allocs == 2 && g_frees == 1); // regrowth frees the old one
        PinnedBuffer p, q;
        CHECK(p.reserve(10) == hipSuccess && q.reserve(20) == hipSuccess);
        q = std::move(p); // what q held is freed, p is empty
        CHECK(!p && q.bytes() == 10 && g_frees == 2);
        q = std::move(q); // self-move keeps it
        CHECK(q && q.bytes() == 10 && g_frees == 2);
        Event e, f;
        CHECK(!e.get() && e.create(2) == hipSuccess && e.get());
        hipEvent_t was = e.get();
        CHECK(e.create(2) == hipSuccess && e.get() == was); // created once, lazily
        f = std::move(e);
        CHECK(!e.get() && f.get() == was);
        Stream s;
        CHECK(s.create() == hipSuccess && s.get());
        Stream t(std::move(s));
        CHECK(!s.get() && t.get());
        t.reset();
        t.reset(); // a second reset frees nothing
        CHECK(!t.get() && g_badFrees == 0);
    }
    CHECK(balanced());

    // 2. reserve with fewer bytes allocates nothing
    {
        DeviceBuffer a;
        CHECK(a.reserve(4096) == hipSuccess);
        void *p = a.get();
        const int allocs = g_allocs, frees = g_frees;
        CHECK(a.reserve(4096) == hipSuccess && a.reserve(1) == hipSuccess && a.reserve(0) == hipSuccess);
        CHECK(a.get() == p && a.bytes() == 4096 && g_allocs == allocs && g_frees == frees);
    }
    CHECK(balanced());

    // 3. a failing allocation leaves the owner empty, and the next reserve works
    {
        PinnedBuffer a;
        CHECK(a.reserve(64) == hipSuccess);
        g_failAfter = 0;
        CHECK(a.reserve(128) == hipErrorOutOfMemory && !a && a.get() == NULL && a.bytes() == 0);
        CHECK(a.reserve(32) == hipSuccess && a && a.bytes() == 32);
        Event e;
        g_failAfter = 0;
        CHECK(e.create(0) == hipErrorOutOfMemory && !e.get());
        CHECK(e.create(0) == hipSuccess && e.get());
        Stream s;
        g_failAfter = 0;
        CHECK(s.create() == hipErrorOutOfMemory && !s.get());
    }
    CHECK(balanced());

    // 5. a struct of owners that is destroyed half-built frees what exists and nothing else
    for (int built = 0; built <= 6; built++)
    {
        const int before = g_allocs;
        {
            Slot *slot = new Slot();
            g_failAfter = built; // the (built + 1)-th of the six fails
            hipError_t e;
            const bool ok = (e = slot->pinnedIn.reserve(16)) == hipSuccess && (e = slot->pinnedOut.reserve(16)) == hipSuccess &&
                            (e = slot->dIn.reserve(16)) == hipSuccess && (e = slot->dOut.reserve(16)) == hipSuccess &&
                            (e = slot->stream.create()) == hipSuccess && (e = slot->done.create(2)) == hipSuccess;
            g_failAfter = -1;
            CHECK(ok == (built == 6) && g_allocs - before == built && (int)g_live.size() == built);
            delete slot;
        }
        CHECK(balanced());
    }

    if (g_failed)
        return 1;
    printf("ok allocs=%d frees=%d\n", g_allocs, g_frees);
    return 0;
}
