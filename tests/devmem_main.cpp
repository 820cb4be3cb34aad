// devmem_main.cpp - the owner type of device memory (thetis_amd/csrc/swe2d_devmem.h: DevArray) over a funnel of malloc / free, on the
// host: tests/test_devmem.py compiles this with the address and undefined-behaviour sanitizers and runs it once.
//
// The funnel here counts live bytes and live allocations like the library's and can fail the n-th allocation from now.  Sub-cases:
//   * alloc / ensure / reset; alloc to the same size (kept) and to another (freed first); ensure on a full array (kept);
//   * move construction, move assignment onto an empty and onto a full target, and onto itself;
//   * a std::vector of a struct with three arrays growing past its capacity (the arrays keep their addresses);
//   * a build function that allocates three arrays into a local struct and moves it into place at the end, made to fail at the first,
//     second and third allocation: the target is as it was, nothing of the attempt is left.
// After every sub-case the live counters are zero.  Prints "ok N" (N sub-cases) and returns 0; a difference: its message on stderr,
// status 3.  A leak or a double free is the sanitizer's report on stderr.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };        // what swe2d_devmem.h names; the library has the HIP runtime's
#include "../thetis_amd/csrc/swe2d_devmem.h"

static size_t g_bytes = 0, g_allocs = 0;
static int g_fail_in = 0;                                           // > 0: the g_fail_in-th allocation from now fails

int swe_dev_alloc(void **p, size_t bytes)
{
    *p = nullptr;
    if (g_fail_in > 0 && --g_fail_in == 0) return (int)hipErrorOutOfMemory;
    size_t *q = static_cast<size_t *>(malloc(bytes + 16));          // the size in front, as the library keeps it in a map
    if (!q) return (int)hipErrorOutOfMemory;
    q[0] = bytes;
    g_bytes += bytes; g_allocs++;
    *p = reinterpret_cast<char *>(q) + 16;
    return (int)hipSuccess;
}

void swe_dev_free(void *p)
{
    if (!p) return;
    size_t *q = reinterpret_cast<size_t *>(static_cast<char *>(p) - 16);
    g_bytes -= q[0]; g_allocs--;
    free(q);
}

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 3; } } while (0)
#define CHECK_NONE_LIVE() CHECK(g_bytes == 0 && g_allocs == 0, "%zu bytes in %zu allocations are live", g_bytes, g_allocs)

struct Three {
    bool live = false;
    DevArray<int> cell;
    DevArray<double> weight, out;
};

// as the library's creators: into a local, moved into place at the end; any failure returns on the spot
static hipError_t build_three(Three &target, size_t n)
{
    Three t;
    hipError_t e;
    if ((e = t.cell.alloc(n)) != hipSuccess) return e;
    if ((e = t.weight.alloc(3*n)) != hipSuccess) return e;
    if ((e = t.out.alloc(5*n)) != hipSuccess) return e;
    t.live = true;
    target = std::move(t);
    return hipSuccess;
}

int main()
{
    int cases = 0;
    {   // alloc / ensure / reset
        DevArray<double> a;
        CHECK(!a && a.get() == nullptr && a.size() == 0, "a fresh array is not empty");
        CHECK(a.alloc(7) == hipSuccess && a && a.size() == 7 && g_bytes == 56 && g_allocs == 1, "alloc(7)");
        double *p = a;
        for (int i = 0; i < 7; i++) p[i] = i;                       // (all of it is writable)
        CHECK(a.alloc(7) == hipSuccess && a.get() == p && g_allocs == 1, "alloc to the same size must keep the array");
        CHECK(a.ensure(9) == hipSuccess && a.get() == p && a.size() == 7, "ensure on a full array must keep it");
        CHECK(a.alloc(9) == hipSuccess && a.size() == 9 && g_bytes == 72 && g_allocs == 1, "alloc to another size frees the old one first");
        a[8] = 1.0;
        a.reset();
        CHECK(!a && a.size() == 0, "reset");
        a.reset();                                                  // (twice: nothing)
        CHECK(a.ensure(3) == hipSuccess && a.size() == 3 && g_bytes == 24, "ensure on an empty array allocates");
        g_fail_in = 1;
        CHECK(a.alloc(4) == hipErrorOutOfMemory && !a && a.size() == 0, "a failed alloc leaves the array empty");
        CHECK_NONE_LIVE();
        CHECK(a.ensure(2) == hipSuccess, "ensure after a failure");
    }                                                               // (the destructor frees)
    CHECK_NONE_LIVE(); cases++;
    {   // moves
        DevArray<int> a, b, c;
        CHECK(a.alloc(4) == hipSuccess && b.alloc(6) == hipSuccess, "alloc");
        int *pa = a, *pb = b;
        DevArray<int> d(std::move(a));
        CHECK(!a && a.size() == 0 && d.get() == pa && d.size() == 4 && g_allocs == 2, "move construction");
        c = std::move(d);
        CHECK(!d && c.get() == pa && c.size() == 4 && g_allocs == 2, "move assignment onto an empty target");
        c = std::move(b);
        CHECK(!b && c.get() == pb && c.size() == 6 && g_allocs == 1 && g_bytes == 24, "move assignment onto a full target frees what it held");
        DevArray<int> &self = c;
        c = std::move(self);
        CHECK(c.get() == pb && c.size() == 6 && g_allocs == 1, "move assignment onto itself");
        c[5] = 1;
        std::swap(c, a);
        CHECK(!c && a.get() == pb && a.size() == 6 && g_allocs == 1, "swap");
        c = DevArray<int>();
        a = DevArray<int>();                                        // (resetting a slot by assignment)
        CHECK_NONE_LIVE();
    }
    CHECK_NONE_LIVE(); cases++;
    {   // a vector of a struct with three arrays, grown past its capacity
        std::vector<Three> v;
        std::vector<int *> first;
        for (int i = 0; i < 40; i++) {
            Three t;
            CHECK(build_three(t, (size_t)i + 1) == hipSuccess, "build_three");
            first.push_back(t.cell.get());
            v.push_back(std::move(t));
        }
        CHECK(g_allocs == 120, "%zu allocations live, 120 expected", g_allocs);
        for (int i = 0; i < 40; i++) {
            CHECK(v[i].live && v[i].cell.get() == first[i] && v[i].cell.size() == (size_t)i + 1 && v[i].out.size() == 5*((size_t)i + 1), "element %d moved wrongly", i);
            v[i].cell[i] = i; v[i].out[5*i + 4] = 1.0;
        }
        v[7] = Three();                                             // a destroyed set leaves an empty slot
        CHECK(g_allocs == 117 && !v[7].live && !v[7].cell, "resetting a slot");
        v.erase(v.begin() + 3);
        CHECK(g_allocs == 114 && v[3].cell.get() == first[4], "erase");
    }
    CHECK_NONE_LIVE(); cases++;
    for (int fail_at = 1; fail_at <= 3; fail_at++) {   // a build that fails at its first, second, third allocation
        Three target;
        CHECK(build_three(target, 2) == hipSuccess && g_allocs == 3, "build_three");
        const int *held = target.cell.get();
        const size_t bytes = g_bytes;
        g_fail_in = fail_at;
        CHECK(build_three(target, 100) == hipErrorOutOfMemory, "allocation %d was to fail", fail_at);
        CHECK(g_fail_in == 0 && g_allocs == 3 && g_bytes == bytes && target.live && target.cell.get() == held && target.cell.size() == 2,
              "a build that failed at allocation %d left something or touched its target", fail_at);
        CHECK(build_three(target, 100) == hipSuccess && g_allocs == 3 && target.cell.size() == 100 && target.cell.get() != held, "the next build replaces the target");
        target = Three();
        CHECK_NONE_LIVE(); cases++;
    }
    printf("ok %d\n", cases);
    return 0;
}
