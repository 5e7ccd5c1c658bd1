// packer_bind.cpp — stand-alone host program over osg_packer's pointer binding (csrc/match_common.h, test-only):
// bind / bind_rows / bind_at / relocate / clear against a pack made with plain add / add_rows / reserve.
// Plain host C++ (the HIP headers are only declarations here): tests/test_packer_bind.py builds it with
// -fsanitize=address,undefined and runs it directly; it prints "ok".
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "match_common.h"

// the two library functions the headers call (runtime.hip)
int osg_set_error(osg_ctx *, int code, const char *, ...) { return code; }
void osg_parallel_run(int n, int, void (*fn)(void *, int), void *arg)
{
    for (int i = 0; i < n; i++) fn(arg, i);
}

#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s (line %d)\n", #cond, __LINE__);         \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// kernel arguments as the units declare them: scalars between pointer fields of several types
struct Args {
    int n;
    const float *x;
    const uint8_t *desc;    // row gather
    const int32_t *none;    // null source
    const int32_t *empty;   // zero bytes
    float th;
    const float *region;    // inside a reserved region
    const float *alias;     // the offset of x again
    const uint8_t *foreign; // never bound: a caller's device pointer
    int32_t *out;           // never bound: set by the caller after relocate
};

static bool all_null(const Args &A)
{
    return !A.x && !A.desc && !A.none && !A.empty && !A.region && !A.alias && !A.foreign && !A.out;
}

int main()
{
    std::vector<float> x(70), y(33);
    std::vector<uint8_t> desc(64 * 32);
    for (size_t i = 0; i < x.size(); i++) x[i] = (float)i;
    for (size_t i = 0; i < y.size(); i++) y[i] = -(float)i;
    for (size_t i = 0; i < desc.size(); i++) desc[i] = (uint8_t)(i * 7);
    const std::vector<int32_t> idx = {63, 0, 5, 5, 17};
    const int32_t z = 0;
    uint8_t foreign[4];
    char *const dev = (char *)(uintptr_t)0x7f0000001000ull;  // a device base: never dereferenced

    // the reference pack: plain add / add_rows / reserve, in the order the bound pack uses
    osg_packer ref;
    const size_t r_x = ref.add(x.data(), 4 * x.size());
    const size_t r_desc = ref.add_rows(desc.data(), idx.data(), idx.size(), 32);
    const size_t r_none = ref.add(nullptr, 16), r_empty = ref.add(&z, 0);
    const size_t r_res = ref.reserve(300);
    const size_t r_y = ref.add(y.data(), 4 * y.size());
    EXPECT(r_x == 0 && r_desc == 512 && r_none == SIZE_MAX && r_empty == SIZE_MAX && r_res == 768 && r_y == 1280);

    // a batch of three: the middle problem binds nothing
    osg_packer pk;
    {
        auto args = std::make_unique<std::vector<Args>>(3);  // sized before the first bind
        std::vector<Args> &a = *args;
        a[0].foreign = a[2].foreign = foreign;
        a[0].n = 70, a[0].th = 0.5f;
        const size_t o_x = pk.bind(a[0].x, x.data(), 4 * x.size());
        const size_t o_desc = pk.bind_rows(a[0].desc, desc.data(), idx.data(), idx.size(), 32);
        const size_t o_none = pk.bind(a[0].none, nullptr, 16), o_empty = pk.bind(a[0].empty, &z, 0);
        const size_t o_res = pk.reserve(300);
        pk.bind_at(a[0].region, o_res + 16);
        pk.bind_at(a[0].alias, o_x);
        pk.bind_at(a[0].none, SIZE_MAX);  // an absent offset binds nothing
        const size_t o_y = pk.bind(a[2].x, y.data(), 4 * y.size());
        EXPECT(o_x == r_x && o_desc == r_desc && o_none == r_none && o_empty == r_empty && o_res == r_res && o_y == r_y);
        EXPECT(pk.total == ref.total && pk.total == 1536 && pk.items.size() == ref.items.size());
        // a bound field is null until relocate; an unbound one is as the caller left it
        EXPECT(!a[0].x && !a[0].desc && !a[0].region && !a[0].alias && !a[2].x && a[0].foreign == foreign);
        std::vector<char> b_ref(ref.total, (char)0x55), b_pk(pk.total, (char)0x55), b_par(pk.total, (char)0x55);
        ref.fill(b_ref.data());
        pk.fill(b_pk.data());
        pk.fill_parallel(b_par.data(), 4);
        EXPECT(b_ref == b_pk && b_ref == b_par);
        EXPECT(std::memcmp(b_pk.data() + o_desc + 32, desc.data(), 32) == 0);  // row 1 of the gather is source row 0

        pk.relocate(dev);
        EXPECT((const char *)a[0].x == dev + o_x && (const char *)a[0].desc == dev + o_desc);
        EXPECT(a[0].none == nullptr && a[0].empty == nullptr);
        EXPECT((const char *)a[0].region == dev + o_res + 16);
        EXPECT(a[0].alias == a[0].x);
        EXPECT(a[0].foreign == foreign && a[2].foreign == foreign && a[0].out == nullptr);
        EXPECT(a[0].n == 70 && a[0].th == 0.5f);
        EXPECT(all_null(a[1]) && a[1].n == 0 && a[1].th == 0.f);
        EXPECT((const char *)a[2].x == dev + o_y && !a[2].desc && !a[2].region && !a[2].alias);
    }  // the first round's structs are freed here

    // a second round in the same packer: clear() drops every binding of the first
    const size_t cap_items = pk.items.capacity(), cap_bound = pk.bound.capacity();
    pk.clear();
    EXPECT(pk.total == 0 && pk.items.empty() && pk.bound.empty());
    EXPECT(pk.items.capacity() == cap_items && pk.bound.capacity() == cap_bound);
    Args one{};
    const size_t o2 = pk.bind(one.x, y.data(), 4 * y.size());
    pk.bind_at(one.alias, o2);
    pk.relocate(dev + 4096);  // a stale binding would write into the freed vector: an ASan error
    EXPECT(o2 == 0 && pk.total == 256 && (const char *)one.x == dev + 4096 && one.alias == one.x && !one.desc);
    std::printf("ok\n");
    return 0;
}
