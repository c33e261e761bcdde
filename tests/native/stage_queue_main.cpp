// stage_queue_main.cpp -- the staging queue's protocol (oarfish_amd/csrc/oem_stage_queue.h) on the host, with a counting
// allocator in the place of page-locked memory: built by tests/test_stage_queue.py once under ThreadSanitizer and once
// under AddressSanitizer + UBSan.  Batches are 1 - 64 "records" of 8 bytes, filled with a pattern of their ticket.
// Prints one "ok <scenario>" line per scenario; the first failed check ends the program with status 1.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../oarfish_amd/csrc/oem_stage_queue.h"

using namespace oem;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

namespace {

constexpr int kRefused = 7, kFinished = 11; // the owner's status codes

struct Latch {
    std::mutex mu;
    std::condition_variable cv;
    bool is_open = false;
    void open()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            is_open = true;
        }
        cv.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return is_open; });
    }
};

// malloc that counts, fails its fail_at-th request (from 1; 0: never) and logs what it is asked to free
struct Counting {
    std::mutex mu;
    uint64_t requests = 0, allocs = 0, releases = 0, fail_at = 0;
    std::vector<size_t> released; // the capacities, in order
    std::function<void()> on_fail;
    StageAlloc alloc()
    {
        return [this](size_t bytes, StageMem *m) {
            bool fails;
            {
                std::lock_guard<std::mutex> lk(mu);
                fails = ++requests == fail_at;
                if (!fails) ++allocs;
            }
            if (fails) {
                if (on_fail) on_fail();
                return false;
            }
            m->p = malloc(bytes);
            m->pinned = false;
            return m->p != nullptr;
        };
    }
    StageRelease release()
    {
        return [this](StageMem &m) {
            std::lock_guard<std::mutex> lk(mu);
            ++releases;
            released.push_back(m.bytes);
            free(m.p);
        };
    }
    void balanced()
    {
        std::lock_guard<std::mutex> lk(mu);
        CHECK(allocs == releases);
    }
};

struct Batch : StageBatch {
    int tag = 0; // what the owner's initialiser sets
};
using Queue = StageQueue<Batch>;

inline size_t cap_of(uint64_t n) { return 8 * n + (8 * n) / 8 + 4096; }
inline uint64_t pattern(uint64_t ticket, uint64_t i) { return ticket * 0x9E3779B97F4A7C15ull + i * 0x100000001B3ull + 1; }

// The owner of a queue under test: its status (under q.mu), what its worker saw, and the counts the scenarios wait for.
struct Owner {
    Queue q;
    int status_rc = 0;     // (q.mu)
    bool finished = false; // (q.mu)
    std::atomic<int> blocked_seen{0}, told{0};
    std::vector<uint64_t> seen_ticket;
    std::vector<bool> seen_skip;
    uint64_t rec_sum = 0;
    Latch *hold_ticket0 = nullptr;            // process waits here with ticket 0 in hand

    Owner(uint64_t max_staged, size_t pool_cap, Counting &c) : q(max_staged, pool_cap, c.alloc(), c.release())
    {
        q.start([this](Batch &b, bool skip) {
            if (hold_ticket0 && b.ticket == 0) hold_ticket0->wait();
            CHECK(b.ticket == seen_ticket.size()); // ticket order
            CHECK(b.rec_base == rec_sum);          // the running sum in ticket order
            CHECK(b.tag == 42);
            CHECK(b.ready);
            rec_sum += b.n_records;
            seen_ticket.push_back(b.ticket);
            seen_skip.push_back(skip);
            if (b.unstaged) CHECK(skip && !b.mem.p);
            if (!skip) { // every byte is the pattern of its ticket
                CHECK(b.mem.p && b.mem.bytes >= 8 * b.n_records);
                for (uint64_t i = 0; i < b.n_records; ++i) {
                    uint64_t v;
                    memcpy(&v, (const char *)b.mem.p + 8 * i, 8);
                    CHECK(v == pattern(b.ticket, i));
                }
            }
            {
                std::lock_guard<std::mutex> lk(q.mu);
                CHECK(q.pool.idle.size() <= q.pool.capacity);
            }
        });
    }
    // one push of n records as a session makes it: the status, the initialiser, the pattern
    int push(uint64_t n, uint64_t *out_ticket = nullptr, Latch *hold_fill = nullptr, std::atomic<int> *fill_entered = nullptr)
    {
        uint64_t ticket = ~0ull;
        return q.push(
            n, 8 * n,
            [&](std::unique_lock<std::mutex> &lk) {
                CHECK(lk.owns_lock());
                if (status_rc) return status_rc; // the sticky status comes before "finished"
                if (finished) return kFinished;
                if (q.staged_records != 0 && q.staged_records + n > q.max_staged) ++blocked_seen; // (it will wait)
                return 0;
            },
            [&](Batch &b) {
                ticket = b.ticket;
                b.tag = 42;
            },
            [&](char *mem) {
                if (fill_entered) ++*fill_entered;
                if (hold_fill) hold_fill->wait();
                for (uint64_t i = 0; i < n; ++i) {
                    const uint64_t v = pattern(ticket, i);
                    memcpy(mem + 8 * i, &v, 8);
                }
            },
            out_ticket);
    }
    uint64_t tickets()
    {
        std::lock_guard<std::mutex> lk(q.mu);
        return q.next_ticket;
    }
    uint64_t staged()
    {
        std::lock_guard<std::mutex> lk(q.mu);
        return q.staged_records;
    }
};

void wait_for(const std::atomic<int> &v, int at_least)
{
    while (v.load() < at_least) std::this_thread::yield();
}

// 1. four pushing threads, 50 batches each, a budget of 128 records
void ticket_order_and_payload()
{
    Counting c;
    {
        Owner o(128, 4, c);
        Latch first;
        o.hold_ticket0 = &first;
        std::vector<std::vector<uint64_t>> got(4);
        std::vector<std::thread> th;
        for (int t = 0; t < 4; ++t)
            th.emplace_back([&, t] {
                uint64_t x = 88172645463325252ull + 977 * t;
                for (int k = 0; k < 50; ++k) {
                    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
                    uint64_t ticket = ~0ull;
                    CHECK(o.push(1 + x % 64, &ticket) == 0);
                    got[t].push_back(ticket);
                }
            });
        // the worker sits on ticket 0 until a push has found no room, and a little longer: the blocked time is not 0
        wait_for(o.blocked_seen, 1);
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
        first.open();
        for (auto &t : th) t.join();
        o.q.close();
        std::vector<int> issued(200, 0);
        for (const auto &g : got)
            for (size_t k = 0; k < g.size(); ++k) {
                CHECK(g[k] < 200 && ++issued[g[k]] == 1);
                CHECK(k == 0 || g[k] > g[k - 1]); // a thread's own tickets ascend
            }
        CHECK(o.seen_ticket.size() == 200 && o.tickets() == 200 && o.staged() == 0);
        for (bool s : o.seen_skip) CHECK(!s);
        std::lock_guard<std::mutex> lk(o.q.mu);
        CHECK(o.q.blocked_us > 0 && o.q.total_records == o.rec_sum && o.q.pushing == 0);
    }
    c.balanced();
    puts("ok ticket order and payload");
}

// 2. with nothing staged a batch larger than the budget is admitted; the next push waits for it
void oversized_batch()
{
    Counting c;
    {
        Owner o(8, 2, c);
        Latch first;
        o.hold_ticket0 = &first;
        CHECK(o.push(20) == 0 && o.staged() == 20);
        uint64_t ticket = ~0ull;
        std::thread next([&] { CHECK(o.push(1, &ticket) == 0); });
        wait_for(o.blocked_seen, 1);
        CHECK(o.tickets() == 1); // it has no ticket while it waits
        first.open();
        next.join();
        CHECK(ticket == 1);
        o.q.close();
        CHECK(o.seen_ticket.size() == 2 && o.staged() == 0);
    }
    c.balanced();
    puts("ok oversized batch");
}

// 3. the allocator fails on request k (k = 1: the first batch of all; k = 2: behind a staged one)
void allocator_failure(uint64_t k)
{
    Counting c;
    {
        Owner o(16, 2, c);
        c.fail_at = k;
        c.on_fail = [&] { // the owner is told where the allocation fails: its session is stuck from here on
            std::lock_guard<std::mutex> lk(o.q.mu);
            o.status_rc = kRefused;
            ++o.told;
        };
        Latch first;
        o.hold_ticket0 = &first;
        for (uint64_t t = 0; t + 1 < k; ++t) CHECK(o.push(4) == 0);
        int rc[2] = {0, 0};
        std::vector<std::thread> blocked;
        if (k > 1) { // two pushes that find no room while the failing one still does
            for (int t = 0; t < 2; ++t) blocked.emplace_back([&, t] { rc[t] = o.push(16); });
            wait_for(o.blocked_seen, 2);
        }
        uint64_t ticket = 77;
        CHECK(o.push(4, &ticket) == kStageNoMemory && ticket == 77);
        CHECK(o.told == 1 && o.tickets() == k);
        if (k > 1) CHECK(o.staged() == 4 * k); // its records leave the budget with the worker, once
        first.open();
        for (auto &t : blocked) t.join();
        if (k > 1) CHECK(rc[0] == kRefused && rc[1] == kRefused);
        CHECK(o.push(1) == kRefused); // sticky
        o.q.close();
        CHECK(o.seen_ticket.size() == k && o.seen_skip[k - 1] && o.tickets() == k && o.staged() == 0 && o.told == 1);
        for (uint64_t t = 0; t + 1 < k; ++t) CHECK(!o.seen_skip[t]);
    }
    c.balanced();
    printf("ok allocator failure %llu\n", (unsigned long long)k);
}

// 4. the owner's status starts failing while three pushes wait: all three return it, none takes a ticket
void status_error_while_blocked()
{
    Counting c;
    {
        Owner o(8, 2, c);
        Latch first;
        o.hold_ticket0 = &first;
        CHECK(o.push(8) == 0);
        int rc[3] = {0, 0, 0};
        std::vector<std::thread> th;
        for (int t = 0; t < 3; ++t) th.emplace_back([&, t] { rc[t] = o.push(1 + t); });
        wait_for(o.blocked_seen, 3);
        {
            std::lock_guard<std::mutex> lk(o.q.mu);
            o.status_rc = kRefused;
        }
        o.q.wake_pushers();
        for (auto &t : th) t.join();
        CHECK(rc[0] == kRefused && rc[1] == kRefused && rc[2] == kRefused && o.tickets() == 1 && o.staged() == 8);
        CHECK(o.q.pushes_in_flight() == 0);
        first.open();
        o.q.close();
        CHECK(o.seen_ticket.size() == 1 && o.staged() == 0);
    }
    c.balanced();
    puts("ok status error while blocked");
}

// 5. a push is in flight while its fill runs
void push_in_flight()
{
    Counting c;
    {
        Owner o(64, 2, c);
        Latch fill;
        std::atomic<int> entered{0};
        CHECK(o.q.pushes_in_flight() == 0);
        std::thread th([&] { CHECK(o.push(3, nullptr, &fill, &entered) == 0); });
        wait_for(entered, 1);
        CHECK(o.q.pushes_in_flight() != 0 && o.tickets() == 1 && o.seen_ticket.empty()); // (unready: the worker waits)
        fill.open();
        th.join();
        CHECK(o.q.pushes_in_flight() == 0);
        o.q.close();
        CHECK(o.seen_ticket.size() == 1);
    }
    c.balanced();
    puts("ok push in flight");
}

// 6. / 7. close lets the worker run every staged batch, cancel makes it skip every one; a later push is refused
void close_or_cancel(bool cancel)
{
    Counting c;
    {
        Owner o(1024, 2, c);
        Latch fill; // ticket 0 stays unready, so all five batches are staged when the queue is stopped
        std::atomic<int> entered{0};
        std::thread first([&] { CHECK(o.push(5, nullptr, &fill, &entered) == 0); });
        wait_for(entered, 1);
        for (int k = 1; k < 5; ++k) CHECK(o.push(5 + k) == 0);
        CHECK(o.staged() == 5 + 6 + 7 + 8 + 9 && o.seen_ticket.empty());
        std::thread opener([&] {
            for (;;) {
                {
                    std::lock_guard<std::mutex> lk(o.q.mu);
                    if (o.q.stop) break;
                }
                std::this_thread::yield();
            }
            fill.open();
        });
        {
            std::lock_guard<std::mutex> lk(o.q.mu);
            o.finished = true;
        }
        if (cancel) o.q.cancel();
        else o.q.close();
        first.join();
        opener.join();
        CHECK(o.seen_ticket.size() == 5 && o.staged() == 0);
        for (bool s : o.seen_skip) CHECK(s == cancel);
        CHECK(o.push(1) == kFinished && o.tickets() == 5);
    }
    c.balanced();
    puts(cancel ? "ok cancel" : "ok close");
}

// 8. the pool: reuse, its capacity, and which allocation goes when it is full
void pool()
{
    { // equal-sized batches against a budget of two of them: the third push always finds an idle allocation
        Counting c;
        {
            Owner o(16, 4, c);
            for (int k = 0; k < 50; ++k) CHECK(o.push(8) == 0);
            o.q.close();
            CHECK(o.seen_ticket.size() == 50);
            std::lock_guard<std::mutex> lk(c.mu);
            CHECK(c.allocs <= 2 && c.requests == c.allocs);
        }
        c.balanced();
    }
    const uint64_t sizes[2][3] = {{1, 32, 64}, {64, 32, 1}};
    for (const auto &sz : sizes) { // three allocations come back to a pool of two: the smallest goes, incoming or not
        Counting c;
        {
            Owner o(1024, 2, c);
            Latch first;
            o.hold_ticket0 = &first;
            for (uint64_t n : sz) CHECK(o.push(n) == 0);
            first.open();
            o.q.close();
            std::lock_guard<std::mutex> lk(o.q.mu);
            std::lock_guard<std::mutex> lk2(c.mu);
            CHECK(c.allocs == 3 && o.q.pool.idle.size() == 2);
            CHECK(c.released.size() == 1 && c.released[0] == cap_of(1));
            for (const StageMem &m : o.q.pool.idle) CHECK(m.bytes == cap_of(32) || m.bytes == cap_of(64));
            // best fit: the smaller of the two that hold the request
            StageMem m = o.q.pool.take(8 * 32);
            CHECK(m.bytes == cap_of(32));
            o.q.pool.give(m);
            CHECK(!m.p && o.q.pool.idle.size() == 2);
            CHECK(!o.q.pool.take(cap_of(64) + 1).p);
        }
        c.balanced();
    }
    puts("ok pool");
}

} // namespace

int main()
{
    ticket_order_and_payload();
    oversized_batch();
    allocator_failure(1);
    allocator_failure(2);
    status_error_while_blocked();
    push_in_flight();
    close_or_cancel(false);
    close_or_cancel(true);
    pool();
    return 0;
}
