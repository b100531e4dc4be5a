// fnn_engine_buffers_main.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Stand-alone check of the engine's device-buffer bookkeeping (fnn_engine.h: create / comm_set / destroy) over a counting
// backend: alloc records every size it is asked for and can be told to fail at its k-th call, free checks that the pointer
// is live.  For n = 0, 3, 5, 9 and six configurations (Canonical without / with a screening copy, Relaxed, several ranks,
// several ranks set twice, several ranks set and taken back) the program checks that
//   * nothing is live after destroy();
//   * a failure at the k-th allocation, for every k, makes create or comm_set return FNN_ENOMEM, and nothing is live after
//     destroy() either.
// With --print it writes every configuration's allocation sequence (index, bytes) to stdout: the order and the byte counts
// fix the device addresses, so two versions of fnn_engine.h must print the same.  It has its own main: it can be built with
// -fsanitize=address,undefined and run directly (tests/test_engine_buffers.py does both).
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../../fastneighbornet_amd/csrc/fnn_engine.h"

using namespace fnn;

struct CountingBackend {
    static constexpr int64_t kRowPad = 32;
    static constexpr int64_t kColPad = 2048;
    int32_t min_n = INT_MAX;  // taxa from which the screening copy exists
    int fail_at = 0;          // > 0: the fail_at-th alloc returns NULL
    int calls = 0, bad_free = 0;
    std::vector<size_t> asked;
    std::set<void*> live;
    int32_t screen_min_n() const { return min_n; }
    void set_problem_size(int32_t) {}
    std::string err() const { return "counting"; }
    int32_t open(int32_t) { return FNN_OK; }
    void close() {}
    void* alloc(size_t b) {
        asked.push_back(b);
        if (++calls == fail_at) return nullptr;
        void* p = std::malloc(16);
        live.insert(p);
        return p;
    }
    void free(void* p) {
        if (!p) return;
        if (!live.erase(p)) { bad_free++; return; }
        std::free(p);
    }
    size_t max_records(int32_t) { return 1; }
    int32_t memset(void*, int, size_t) { return FNN_OK; }
};

struct Config {
    const char* name;
    int32_t mode, min_n;
    int ncomm;
    int32_t worlds[2][2];  // {world, rank} of up to two comm_set(2, ..) calls
};
static const Config kConfigs[] = {
    {"canonical", FNN_MODE_CANONICAL, INT_MAX, 0, {}},
    {"canonical+screen", FNN_MODE_CANONICAL, 8, 0, {}},
    {"relaxed", FNN_MODE_RELAXED, 8, 0, {}},
    {"ranks(3)", FNN_MODE_CANONICAL, 8, 1, {{3, 1}}},
    {"ranks(3) then ranks(5)", FNN_MODE_CANONICAL, 8, 2, {{3, 1}, {5, 4}}},
    {"ranks(3) then one rank", FNN_MODE_CANONICAL, 8, 2, {{3, 1}, {1, 0}}},
};

struct Outcome {
    int32_t rc = FNN_OK;
    int calls = 0;
    size_t live = 0;
    int bad_free = 0;
    std::vector<size_t> asked;
};

static Outcome run(const Config& c, int32_t n, int fail_at) {
    Engine<CountingBackend> eng;
    eng.be.min_n = c.min_n;
    eng.be.fail_at = fail_at;
    fnn_opts o{};
    o.mode = c.mode;
    Outcome out;
    out.rc = eng.create(n, &o);
    for (int k = 0; k < c.ncomm && out.rc == FNN_OK; k++) out.rc = eng.comm_set(2, c.worlds[k][0], c.worlds[k][1]);
    eng.destroy();
    out.calls = eng.be.calls;
    out.live = eng.be.live.size();
    out.bad_free = eng.be.bad_free;
    out.asked = eng.be.asked;
    for (void* p : eng.be.live) std::free(p);
    return out;
}

int main(int argc, char** argv) {
    const bool print = argc > 1 && !std::strcmp(argv[1], "--print");
    unsetenv("FNN_COMM_FORCE");
    unsetenv("FNN_LDH_PAD");
    unsetenv("FNN_FAULT_ERROR");
    int bad = 0;
    long runs = 0;
    for (const Config& c : kConfigs)
        for (int32_t n : {0, 3, 5, 9}) {
            const Outcome whole = run(c, n, 0);
            runs++;
            if (whole.rc != FNN_OK || whole.live != 0 || whole.bad_free != 0) {
                std::printf("%s, n = %d: rc %d, %zu live, %d bad frees after destroy()\n", c.name, n, whole.rc, whole.live, whole.bad_free);
                bad = 1;
            }
            if (print) {
                std::printf("# %s, n = %d: %d allocations\n", c.name, n, whole.calls);
                for (size_t i = 0; i < whole.asked.size(); i++) std::printf("%zu %zu\n", i, whole.asked[i]);
            }
            for (int k = 1; k <= whole.calls; k++) {
                const Outcome o = run(c, n, k);
                runs++;
                if (o.rc != FNN_ENOMEM || o.calls != k || o.live != 0 || o.bad_free != 0) {
                    std::printf("%s, n = %d, allocation %d of %d fails: rc %d after %d allocations, %zu live, %d bad frees after destroy()\n",
                                c.name, n, k, whole.calls, o.rc, o.calls, o.live, o.bad_free);
                    bad = 1;
                }
            }
        }
    if (bad) return 1;
    if (!print) std::printf("ok: %ld runs\n", runs);
    return 0;
}
