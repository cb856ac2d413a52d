// staging_layout.cpp -- csrc/staging.h without a GPU: the layout rules of Staging against a plain Carver, and one whole round trip
// (put, "upload", "kernel", "download", get) in two heap buffers of exactly host_bytes() and device_bytes().  Built with
// -fsanitize=address,undefined: a block that reaches past either size is a failure.  The only project header is staging.h.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "staging.h"

using namespace orbfe;

namespace {

struct Odd3 { uint8_t b[3]; };
struct Odd12 { uint8_t b[12]; };
struct Odd1196 { uint8_t b[1196]; };  // a record of floats and ints that is no multiple of 8, as orbfe_imu_preint

enum Phase { IN, SCRATCH, OUT, INOUT };

struct Take {
    Phase phase;
    size_t size, n;
};

// one taken block with its type erased: the offset and count Staging gave, and the typed calls bound to it
struct Taken {
    Take t;
    size_t off;
    std::function<uint8_t*(const Staging&)> host, dev;
    std::function<const uint8_t*(const Staging&)> res;
    std::function<void(const Staging&, const void*)> put;
    std::function<void(const Staging&, void*)> get;
};

int failures = 0;
#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond);     \
            printf(__VA_ARGS__);                                      \
            printf("\n");                                             \
            failures++;                                               \
        }                                                             \
    } while (0)

template <class T>
Taken take_as(Staging& st, const Take& t)
{
    Block<T> b;
    switch (t.phase) {
    case IN: b = st.in<T>(t.n); break;
    case SCRATCH: b = st.scratch<T>(t.n); break;
    case OUT: b = st.out<T>(t.n); break;
    default: b = st.inout<T>(t.n); break;
    }
    Taken k;
    k.t = t;
    k.off = b.off;
    if (b.n != t.n || b.bytes() != t.n * sizeof(T) || b.end() != b.off + t.n * sizeof(T)) {
        printf("FAIL the handle of a %zu x %zu block carries n %zu bytes %zu\n", t.n, sizeof(T), b.n, b.bytes());
        failures++;
    }
    k.host = [b](const Staging& s) { return reinterpret_cast<uint8_t*>(s.host(b)); };
    k.dev = [b](const Staging& s) { return reinterpret_cast<uint8_t*>(s.dev(b)); };
    k.res = [b](const Staging& s) { return reinterpret_cast<const uint8_t*>(s.res(b)); };
    k.put = [b](const Staging& s, const void* src) { s.put(b, src); };
    k.get = [b](const Staging& s, void* dst) { s.get(b, dst); };
    return k;
}

Taken take(Staging& st, const Take& t)
{
    switch (t.size) {
    case 1: return take_as<uint8_t>(st, t);
    case 3: return take_as<Odd3>(st, t);
    case 4: return take_as<int>(st, t);
    case 8: return take_as<double>(st, t);
    case 12: return take_as<Odd12>(st, t);
    default: return take_as<Odd1196>(st, t);
    }
}

uint8_t pattern(size_t block, size_t byte, int salt) { return (uint8_t)(block * 37 + byte * 11 + salt); }

void run_script(const char* name, const std::vector<Take>& script)
{
    Staging st;
    Carver c;
    std::vector<Taken> blocks;
    size_t wantIn = 0, wantRes = 0, wantResEnd = 0;
    bool sawRes = false;
    for (const Take& t : script) {
        const size_t o = c.take(t.size * t.n);
        const Taken k = take(st, t);
        CHECK(k.off == o, "%s: block %zu lies at %zu, a plain Carver puts it at %zu", name, blocks.size(), k.off, o);
        if ((t.phase == OUT || t.phase == INOUT) && !sawRes) { sawRes = true; wantRes = o; }
        if (t.phase == IN || t.phase == INOUT) wantIn = c.off;
        if (t.phase == OUT || t.phase == INOUT) wantResEnd = c.off;
        blocks.push_back(k);
    }
    const size_t wantResBytes = sawRes ? wantResEnd - wantRes : 0;
    CHECK(st.inBytes == wantIn, "%s: inBytes %zu, want %zu", name, st.inBytes, wantIn);
    CHECK(st.resBytes == wantResBytes, "%s: resBytes %zu, want %zu", name, st.resBytes, wantResBytes);
    if (sawRes) CHECK(st.oRes == wantRes, "%s: oRes %zu, want %zu", name, st.oRes, wantRes);
    CHECK(st.ordered, "%s: a script in phase order is called unordered", name);
    CHECK(st.device_bytes() == c.off, "%s: device_bytes %zu, the Carver ends at %zu", name, st.device_bytes(), c.off);
    CHECK(st.host_bytes() == st.inBytes + st.resBytes, "%s: host_bytes %zu", name, st.host_bytes());

    // exactly as large as the layout says; calloc(0) may return null, which bind() takes as it is
    uint8_t* hp = static_cast<uint8_t*>(calloc(st.host_bytes(), 1));
    uint8_t* dp = static_cast<uint8_t*>(calloc(st.device_bytes(), 1));
    st.bind(hp, dp);

    // addresses, and no two blocks on one byte: on the device among all of them, on the host among inputs and result mirrors
    for (size_t i = 0; i < blocks.size(); i++) {
        const Taken& a = blocks[i];
        const size_t aBytes = a.t.size * a.t.n;
        CHECK(a.dev(st) == dp + a.off, "%s: dev() of block %zu", name, i);
        if (a.t.phase == IN || a.t.phase == INOUT) {
            CHECK(a.host(st) == hp + a.off, "%s: host() of input block %zu", name, i);
            CHECK(a.off + aBytes <= st.inBytes, "%s: input block %zu ends behind inBytes", name, i);
        }
        if (a.t.phase == OUT || a.t.phase == INOUT) {
            CHECK(a.res(st) == hp + st.inBytes + (a.off - st.oRes), "%s: res() of result block %zu", name, i);
            CHECK(st.inBytes + (a.off - st.oRes) + aBytes <= st.host_bytes(), "%s: the mirror of block %zu ends behind host_bytes", name, i);
        }
        CHECK(a.off + aBytes <= st.device_bytes(), "%s: block %zu ends behind device_bytes", name, i);
        for (size_t j = i + 1; j < blocks.size(); j++) {
            const Taken& b = blocks[j];
            const size_t bBytes = b.t.size * b.t.n;
            if (!aBytes || !bBytes) continue;
            CHECK(a.off + aBytes <= b.off, "%s: blocks %zu and %zu overlap on the device", name, i, j);
        }
    }

    // put -> upload -> the kernel's writes -> download -> get
    for (size_t i = 0; i < blocks.size(); i++) {
        const Taken& a = blocks[i];
        if (a.t.phase != IN && a.t.phase != INOUT) continue;
        std::vector<uint8_t> src(a.t.size * a.t.n);
        for (size_t k = 0; k < src.size(); k++) src[k] = pattern(i, k, 1);
        a.put(st, src.empty() ? nullptr : src.data());
    }
    if (st.inBytes) memcpy(dp, hp, st.inBytes);
    for (size_t i = 0; i < blocks.size(); i++) {
        const Taken& a = blocks[i];
        const size_t bytes = a.t.size * a.t.n;
        if (a.t.phase == IN || a.t.phase == INOUT)
            for (size_t k = 0; k < bytes; k++)
                if (a.dev(st)[k] != pattern(i, k, 1)) {
                    CHECK(false, "%s: input block %zu arrived changed at byte %zu", name, i, k);
                    break;
                }
        if (a.t.phase != IN)  // scratch and results are written on the device
            for (size_t k = 0; k < bytes; k++) a.dev(st)[k] = pattern(i, k, 2);
    }
    if (st.resBytes) memcpy(hp + st.inBytes, dp + st.oRes, st.resBytes);
    for (size_t i = 0; i < blocks.size(); i++) {
        const Taken& a = blocks[i];
        if (a.t.phase != OUT && a.t.phase != INOUT) continue;
        std::vector<uint8_t> dst(a.t.size * a.t.n, 0);
        a.get(st, dst.empty() ? nullptr : dst.data());
        for (size_t k = 0; k < dst.size(); k++)
            if (dst[k] != pattern(i, k, 2)) {
                CHECK(false, "%s: result block %zu came back changed at byte %zu", name, i, k);
                break;
            }
    }
    // an input that is no result keeps what was put: the download does not reach into the inputs
    for (size_t i = 0; i < blocks.size(); i++) {
        const Taken& a = blocks[i];
        if (a.t.phase != IN) continue;
        for (size_t k = 0; k < a.t.size * a.t.n; k++)
            if (a.host(st)[k] != pattern(i, k, 1)) {
                CHECK(false, "%s: the download overwrote input block %zu at byte %zu", name, i, k);
                break;
            }
    }
    free(hp);
    free(dp);
    printf("%s: %zu blocks, in %zu res %zu device %zu host %zu\n", name, blocks.size(), st.inBytes, st.resBytes, st.device_bytes(),
           st.host_bytes());
}

// every size with every count, in one phase
void phase_takes(std::vector<Take>& s, Phase p)
{
    const size_t sizes[] = {1, 4, 8, 3, 12, 1196}, counts[] = {0, 1, 63, 64, 65};
    for (size_t size : sizes)
        for (size_t n : counts) s.push_back(Take{p, size, n});
}

}  // namespace

int main()
{
    std::vector<Take> all, noScratch, noInputs, inout, scratchLast, scratchBetween, empty;
    phase_takes(all, IN); phase_takes(all, SCRATCH); phase_takes(all, OUT);
    phase_takes(noScratch, IN); phase_takes(noScratch, OUT);
    phase_takes(noInputs, SCRATCH); phase_takes(noInputs, OUT);
    phase_takes(inout, IN); inout.push_back(Take{INOUT, 1196, 1}); phase_takes(inout, OUT);   // imu_preintegrate_run's kf
    phase_takes(scratchLast, IN); phase_takes(scratchLast, OUT); phase_takes(scratchLast, SCRATCH);   // the projection tables
    run_script("in+scratch+out", all);
    run_script("no scratch", noScratch);
    run_script("no inputs", noInputs);
    run_script("inout", inout);
    run_script("scratch behind the results", scratchLast);
    phase_takes(scratchBetween, IN); phase_takes(scratchBetween, OUT); phase_takes(scratchBetween, SCRATCH); phase_takes(scratchBetween, OUT);   // match_bow_run's bin
    run_script("scratch between results", scratchBetween);
    run_script("nothing", empty);
    {   // an input behind scratch, behind a result, and an inout that is not the last input: all three are flagged
        Staging a, b, c;
        a.in<int>(3); a.scratch<int>(3); a.in<int>(3);
        b.in<int>(3); b.out<int>(3); b.in<int>(3);
        c.in<int>(3); c.inout<int>(3); c.in<int>(3);
        CHECK(!a.ordered && !b.ordered && !c.ordered, "an input out of phase order is not flagged: %d %d %d", a.ordered, b.ordered, c.ordered);
    }

    // put and get: a null pointer and a zero count are no-ops, a count below the block's copies that many
    Staging st;
    const Block<int> a = st.in<int>(4);
    const Block<int> r = st.out<int>(4);
    std::vector<uint8_t> hp(st.host_bytes(), 0xee), dp(st.device_bytes(), 0);
    st.bind(hp.data(), dp.data());
    const int src[4] = {1, 2, 3, 4};
    st.put(a, nullptr);
    st.put(a, src, 0);
    CHECK(hp[0] == 0xee, "put: a null source or a zero count wrote");
    st.put(a, src, 2);
    CHECK(st.host(a)[0] == 1 && st.host(a)[1] == 2 && hp[8] == 0xee, "put: count 2");
    int dst[4] = {-1, -1, -1, -1};
    st.get(r, nullptr);
    st.get(r, dst, 0);
    CHECK(dst[0] == -1, "get: a zero count wrote");
    memcpy(hp.data() + st.inBytes, src, sizeof src);
    st.get(r, dst, 3);
    CHECK(dst[0] == 1 && dst[2] == 3 && dst[3] == -1, "get: count 3");

    printf(failures ? "staging_layout: %d FAILED\n" : "staging_layout: ok\n", failures);
    return failures ? 1 : 0;
}
