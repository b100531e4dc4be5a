// fnn_feed_emu_main.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The engine's continuous feed (fnn_engine.h: agglomerate_feed) on the CPU.  The backend is the emulation's (fnn_emu.cpp, by
// inclusion) plus the mailbox methods: every launch sequence runs synchronously and files a FeedRec, and a record becomes
// visible to the host only `lag` launches later - a deterministic stand-in for a device that runs behind the host.  Waiting
// for a record lets the "device" catch up: everything filed becomes visible.
//
//   fnn_feed_emu_main --unit                          the record check (fnn_core.h: feed_pick): a torn record, a record of the
//                                                     previous generation and a repeated sequence number are passed over
//   fnn_feed_emu_main <input> [lookahead pairs]       <input>: int32 n, n * n doubles (the matrix), n + 1 int32 (the oracle's
//                                                     order).  Every depth in {1, 2, 16, 1024} with every lag in
//                                                     {0, 1, depth - 1} must give that order, through the feed, with at most
//                                                     `depth` launch sequences behind the last event and a bounded number of
//                                                     launches in all (stalls end).  Prints the stalled sequences it saw.
// It has its own main: it is built plainly and with -fsanitize=address,undefined and run directly (tests/test_feed_emu.py).
#include <cstdio>
#include <deque>
#include <set>

#include "fnn_emu.cpp"

namespace {

struct FeedEmuBackend : EmuBackend {
    int lag = 0;
    bool on = false;
    int32_t gen = 0;
    int64_t seq = 0;
    fnn::FeedRec ring[fnn::FEED_RING] = {};
    std::deque<fnn::FeedWords> filed;  // not yet visible
    int begins = 0;
    int64_t launches = 0, tail = 0, launch_cap = 0, waits = 0;

    void publish(size_t keep) {
        while (filed.size() > keep) {
            const fnn::FeedRec r = __builtin_bit_cast(fnn::FeedRec, filed.front());
            std::memcpy(&ring[r.seq & (fnn::FEED_RING - 1)], &filed.front(), sizeof(fnn::FeedRec));
            filed.pop_front();
        }
    }
    int32_t launch_event(const fnn::Dev& d, int32_t m_bound, bool sched) {
        if (++launches > launch_cap) return FNN_EHIP;  // (a run that never ends is a failure, not a hang)
        if (d.st->done) tail++;
        const int32_t rc = EmuBackend::launch_event(d, m_bound, sched);
        if (on) {
            filed.push_back(fnn::feed_record(*d.st, gen, seq++));
            publish((size_t)lag);
        }
        return rc;
    }
    bool feed_timing_ok() const { return true; }
    bool feed_begin(int64_t first_seq) {
        gen++;
        std::memset(ring, 0, sizeof(ring));
        filed.clear();
        seq = first_seq;
        on = true;
        begins++;
        return true;
    }
    void feed_end() { on = false; }
    bool feed_newest(int64_t seen, fnn::FeedRec* out) const { return fnn::feed_pick(ring, fnn::FEED_RING, gen, seen, out); }
    int32_t feed_wait(int64_t seen, fnn::FeedRec* out, double) {
        waits++;
        publish(0);
        return feed_newest(seen, out) ? FNN_OK : 1;
    }
};

int unit() {
    using namespace fnn;
    int bad = 0;
    auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("record check: %s\n", what); bad = 1; } };
    State st{};
    st.m = 17; st.n_events = 5; st.la_valid = 1; st.la_k = 3; st.la_Kcur = 9; st.n_rx_exact = 2;
    FeedRec ring[FEED_RING] = {};
    FeedRec out{};
    expect(!feed_pick(ring, FEED_RING, 1, -1, &out), "an empty ring holds no record");
    auto put = [&](int slot, int32_t gen, int64_t seq) { const FeedWords w = feed_record(st, gen, seq); std::memcpy(&ring[slot], &w, sizeof w); };
    put(3, 7, 11);
    expect(feed_pick(ring, FEED_RING, 7, 10, &out) && out.seq == 11 && out.m == 17 && out.n_events == 5 && out.la_k == 3 && out.la_Kcur == 9 &&
               out.la_valid == 1 && out.n_rx_exact == 2 && out.done == 0 && out.stall == 0 && out.error == 0,
           "a whole record is taken with its fields");
    expect(!feed_pick(ring, FEED_RING, 7, 11, &out), "a repeated sequence number is passed over");
    expect(!feed_pick(ring, FEED_RING, 7, 12, &out), "an older sequence number is passed over");
    expect(!feed_pick(ring, FEED_RING, 8, -1, &out), "a record of the previous generation is passed over");
    put(4, 7, 12);
    put(5, 6, 13);  // (newer by number, but of another generation)
    expect(feed_pick(ring, FEED_RING, 7, 10, &out) && out.seq == 12, "the newest record of the generation wins");
    // torn: every single word of the newest record replaced by the word of another record, or flipped in one bit
    const FeedWords other = feed_record(st, 7, 99);
    for (int k = 0; k < FEED_WORDS; k++) {
        FeedWords w = feed_record(st, 7, 12);
        if (w.w[k] == other.w[k]) continue;
        w.w[k] = other.w[k];
        std::memcpy(&ring[4], &w, sizeof w);
        expect(feed_pick(ring, FEED_RING, 7, 10, &out) && out.seq == 11, "a torn record is passed over (word of another record)");
        w = feed_record(st, 7, 12);
        w.w[k] ^= 1ULL << (k * 7);
        std::memcpy(&ring[4], &w, sizeof w);
        expect(feed_pick(ring, FEED_RING, 7, 10, &out) && out.seq == 11, "a torn record is passed over (one bit)");
    }
    // half-written over a cleared slot
    {
        FeedWords w = feed_record(st, 7, 20);
        for (int k = FEED_WORDS / 2; k < FEED_WORDS; k++) w.w[k] = 0;
        std::memcpy(&ring[6], &w, sizeof w);
        expect(feed_pick(ring, FEED_RING, 7, 11, &out) == false || out.seq != 20, "a half-written record is passed over");
    }
    if (!bad) std::printf("ok: record check\n");
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--unit")) return unit();
    if (argc < 2) { std::printf("usage: fnn_feed_emu_main --unit | <input> [lookahead pairs]\n"); return 2; }
    unsetenv("FNN_FEED");
    unsetenv("FNN_BATCH");
    unsetenv("FNN_FAULT_ERROR");
    std::FILE* f = std::fopen(argv[1], "rb");
    int32_t n = 0;
    if (!f || std::fread(&n, sizeof n, 1, f) != 1 || n < 4) { std::printf("cannot read %s\n", argv[1]); return 2; }
    std::vector<double> D((size_t)n * (size_t)n);
    std::vector<int32_t> want((size_t)n + 1), got((size_t)n + 1);
    if (std::fread(D.data(), sizeof(double), D.size(), f) != D.size() || std::fread(want.data(), sizeof(int32_t), want.size(), f) != want.size()) {
        std::printf("short input %s\n", argv[1]);
        return 2;
    }
    std::fclose(f);
    fnn_opts o{};
    o.mode = FNN_MODE_CANONICAL;
    if (argc > 3) { o.lookahead = std::atoi(argv[2]); o.lookahead_pairs = std::atoi(argv[3]); }
    int bad = 0, runs = 0;
    long long stalled = 0, hits = 0, waits = 0, events = 0;
    for (int depth : {1, 2, 16, 1024}) {
        std::set<int> lags = {0, 1 < depth ? 1 : 0, depth - 1};
        for (int lag : lags) {
            setenv("FNN_FEED_DEPTH", std::to_string(depth).c_str(), 1);
            fnn::Engine<FeedEmuBackend> eng;
            eng.be.lag = lag;
            // every event is one launch sequence; a stall episode costs at most `depth` more, and there are at most n episodes
            eng.be.launch_cap = (int64_t)n * (depth + 2) + 4096;
            fnn_stats st{};
            int32_t rc = eng.create(n, &o);
            if (rc == FNN_OK) rc = eng.set_rows(0, n, D.data(), n);
            if (rc == FNN_OK) rc = eng.run(got.data(), &st);
            runs++;
            const bool same = rc == FNN_OK && got == want;
            if (!same || eng.be.begins != 1 || eng.be.tail > depth || eng.feed_tail > depth || st.n_events < 1) {
                std::printf("n = %d, depth %d, lag %d: rc %d (%s), order %s, %d feeds, %lld launches (%lld behind the last event, host says %lld), %lld events\n",
                            n, depth, lag, rc, rc == FNN_OK ? "" : fnn::g_last_error.c_str(), same ? "equal" : "DIFFERENT", eng.be.begins,
                            (long long)eng.be.launches, (long long)eng.be.tail, (long long)eng.feed_tail, (long long)st.n_events);
                bad = 1;
            }
            stalled += st.n_stalled_events;
            hits += st.n_window_hits;
            waits += eng.be.waits;
            events = st.n_events;
            eng.destroy();
        }
    }
    if (bad) return 1;
    std::printf("ok: %d runs, %lld stalled sequences, %lld window hits, %lld waits, %lld events per run\n", runs, stalled, hits, waits, events);
    return 0;
}
