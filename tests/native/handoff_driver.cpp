// The RCCL transport's hand-off between the caller's thread and the communicator's worker thread
// (museinference.jl_amd/csrc/comm_handoff.h) without a device, for ThreadSanitizer: a producer that posts the result areas
// round-robin and awaits an area before it posts it again, as the gathered map's start and wait do, and a consumer that takes
// them as the worker does.  What the producer writes before post() the consumer reads after take(), and what the consumer
// writes before enqueued() the producer reads after is_enqueued() -- plain variables, so that a missing ordering is a
// reported race.  Then stop: with the queue empty, and with an entry still in it (which the worker must still serve).
// usage: handoff_driver ROUNDS.  Exit 0 = order and counts as expected.
#include <stdio.h>
#include <stdlib.h>

#include <thread>

#include "../../museinference.jl_amd/csrc/comm_handoff.h"

constexpr int kAreas = 4;
struct Area {
    long count = -1;   // producer -> consumer (the gather's size in the library)
    long done = -1;    // consumer -> producer (the worker's outcome)
};

// `rounds` posts; the last `left` of them are not awaited before stop.  Returns the number of failed checks.
static int run(long rounds, int left) {
    muse::AreaHandoff<kAreas> h;
    Area area[kAreas];
    long served = 0;
    int bad = 0, bad_worker = 0;
    std::thread worker([&] {
        for (int a; h.take(a);) {
            if (a != (int)(served % kAreas) || area[a].count != served) bad_worker += 1;   // FIFO, and the producer's write is visible
            area[a].done = area[a].count;
            served += 1;
            h.enqueued(a);
        }
    });
    auto await = [&](int a, long expect) {
        while (!h.is_enqueued(a)) std::this_thread::yield();
        if (area[a].done != expect) bad += 1;
    };
    for (long r = 0; r < rounds; ++r) {
        const int a = (int)(r % kAreas);
        if (r >= kAreas) await(a, r - kAreas);   // the area's previous gather, before the area is used again
        area[a].count = r;
        h.post(a);
    }
    for (long r = rounds - kAreas < 0 ? 0 : rounds - kAreas; r < rounds - left; ++r) await((int)(r % kAreas), r);
    h.stop();
    worker.join();
    if (served != rounds) bad += 1;   // an entry posted before stop is still served
    for (long r = rounds - left < 0 ? 0 : rounds - left; r < rounds; ++r)
        if (!h.is_enqueued((int)(r % kAreas)) || area[r % kAreas].done != r) bad += 1;
    return bad + bad_worker;
}

int main(int argc, char** argv) {
    const long rounds = argc > 1 ? atol(argv[1]) : 4000;
    int bad = run(rounds, 0);
    for (int rep = 0; rep < 200; ++rep) bad += run(7 + rep % 9, 1 + rep % 3);   // stop with entries pending
    bad += run(0, 0);                                                             // stop before anything was posted
    if (bad) { fprintf(stderr, "%d checks failed\n", bad); return 1; }
    printf("handoff driver ok: %ld rounds\n", rounds);
    return 0;
}
