// oem_stage_queue.h -- the staging queue of the sessions that take batches from several pushing threads and run them on
// ONE worker in ticket order: the records session in its four kinds (oem_records_stream.hip) and
// the parse queue of the barcoded cells sessions (BarcodesStream, oem_cells_barcodes_stream.hip).  Pure host code with no
// HIP in it: the memory comes from two functions of the owner, so tests/native/stage_queue_main.cpp runs the protocol
// under the sanitizers with a counting allocator.
//
//   push      waits under the queue's lock until nothing is staged or the batch fits the budget
//             (staged_records + n <= max_staged; a batch larger than the budget goes alone), asking the owner's status
//             check on every turn and adding the time waited to blocked_us; takes the batch's ticket and the smallest
//             idle allocation that holds it, queues the batch unready and lets the owner's initialiser fill in its own
//             fields; then, outside the lock, allocates where the pool had nothing and lets the owner's fill copy the
//             caller's arrays -- the copies of several pushing threads run side by side; marks the batch ready and wakes
//             the worker.  Where the allocation fails the batch becomes ready with nothing staged (`unstaged`), the
//             worker skips it, and push returns kStageNoMemory: the owner's alloc is the one that saw the failure and
//             makes its session sticky there, before any waiting pusher wakes.
//   worker    takes the front batch once it is ready, or ends when the queue is stopped and empty; calls the owner's
//             process(batch, skip) outside the lock -- skip: the queue is cancelled or the batch is unstaged; the owner
//             adds its sticky status and translates its own exceptions: process must not throw -- then returns the
//             allocation to the pool, takes the batch's records out of the budget and wakes the pushers.
//   close     stops the queue and joins the worker, which runs every staged batch first; cancel does the same with
//             every staged batch skipped.  The owner refuses later pushes through its status check: it sets its own
//             "finished" flag under `mu` before it closes.
//
// `mu` is public because the owner's state that push and process touch (its sticky status, its per-ticket tables) lives
// under the same lock: the status check and the initialiser are called with it held, and an owner takes it wherever it
// reads the queue's counters directly.
//
// Not for the group hand-off of BarcodesStream::cut_groups (cv_groups, groups_in_flight: a bound on groups that share an
// arena, not a queue of batches) and not for oem_cells_stream.hip's own push, which appends cells to an open group arena
// and feeds several workers: both are different protocols.
#pragma once

#include <chrono>
#include <climits>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace oem {

// what push returns for a batch whose staging memory could not be allocated (no owner's status code is INT_MIN)
constexpr int kStageNoMemory = INT_MIN;

// host memory of one staged batch: page-locked where the owner's allocator could have it so
struct StageMem {
    void *p = nullptr;
    size_t bytes = 0;
    bool pinned = false;
};
// alloc(bytes, &m): sets m.p and m.pinned and returns true, or returns false (called outside the lock; the queue sets
// m.bytes).  release(m): frees m.p.
using StageAlloc = std::function<bool(size_t, StageMem *)>;
using StageRelease = std::function<void(StageMem &)>;

// The idle allocations, kept for reuse: page-locking memory costs more than filling it.  (the queue's lock held)
struct StagePool {
    std::vector<StageMem> idle;
    size_t capacity = 0;
    StageRelease release;

    ~StagePool()
    {
        for (StageMem &m : idle) release(m);
    }
    // the smallest idle allocation that holds `bytes`, or an empty one
    StageMem take(size_t bytes)
    {
        size_t best = idle.size();
        for (size_t k = 0; k < idle.size(); ++k)
            if (idle[k].bytes >= bytes && (best == idle.size() || idle[k].bytes < idle[best].bytes)) best = k;
        if (best == idle.size()) return StageMem();
        const StageMem m = idle[best];
        idle.erase(idle.begin() + best);
        return m;
    }
    // m comes back; when the pool is full the smallest allocation, m included, goes
    void give(StageMem &m)
    {
        if (!m.p) return;
        if (idle.size() < capacity) {
            idle.push_back(m);
        } else {
            size_t least = 0;
            for (size_t k = 1; k < idle.size(); ++k)
                if (idle[k].bytes < idle[least].bytes) least = k;
            if (!idle.empty() && idle[least].bytes < m.bytes) std::swap(idle[least], m);
            release(m);
        }
        m = StageMem();
    }
};

// What the queue keeps of a batch; a session derives its Batch with its own fields and layout accessors.
struct StageBatch {
    uint64_t ticket = 0, n_records = 0;
    uint64_t rec_base = 0; // the records of the batches with smaller tickets: the index of its first record in the session
    StageMem mem;          // (none for a batch without bytes, or an unstaged one)
    bool ready = false;    // the pushing thread has finished its copy
    bool unstaged = false; // its staging memory could not be allocated
};

template <typename Batch>
struct StageQueue {
    mutable std::mutex mu;
    // (mu) what the info calls read: tickets issued, records pushed, microseconds pushes have waited for room
    uint64_t next_ticket = 0, total_records = 0, blocked_us = 0;
    uint64_t staged_records = 0; // (mu) records of the batches that are queued or with the worker
    int pushing = 0;             // (mu) pushes between their entry and their batch's ready mark (a waiting push counts twice)
    bool stop = false, cancelled = false; // (mu)
    StagePool pool;                       // (mu)
    const uint64_t max_staged;
    const StageAlloc alloc;
    std::condition_variable cv_work, cv_space;
    std::deque<std::unique_ptr<Batch>> queue; // (mu) ticket order
    std::thread worker;

    StageQueue(uint64_t max_staged_, size_t pool_capacity, StageAlloc alloc_, StageRelease release) : max_staged(max_staged_), alloc(std::move(alloc_))
    {
        pool.capacity = pool_capacity;
        pool.release = std::move(release);
        pool.idle.reserve(pool_capacity); // (give() never allocates)
    }
    StageQueue(const StageQueue &) = delete;
    StageQueue &operator=(const StageQueue &) = delete;
    ~StageQueue()
    {
        cancel();
        for (auto &b : queue) // (only a queue that was never started still holds batches)
            if (b->mem.p) pool.release(b->mem);
    }

    // The one worker: process(Batch &, bool skip), see the head of the file.
    template <typename Process>
    void start(Process process)
    {
        worker = std::thread([this, process]() mutable { work(process); });
    }

    // One batch of n_records records and `bytes` bytes (0: nothing to stage).  status(lk): 0, or the owner's reason to
    // refuse the push, which push returns; called with the lock lk held on every turn of the wait, it may drop lk while
    // it asks elsewhere.  init(batch): the owner's fields, under the lock, once ticket, n_records and rec_base are set;
    // it may throw only before it changes anything of the owner's.  fill(mem): the copy, outside the lock; it must not
    // throw.  Returns 0 with the ticket in *out_ticket (or NULL), status's code, or kStageNoMemory.
    template <typename Status, typename Init, typename Fill>
    int push(uint64_t n_records, size_t bytes, Status &&status, Init &&init, Fill &&fill, uint64_t *out_ticket)
    {
        Batch *b = nullptr;
        {
            std::unique_lock<std::mutex> lk(mu);
            ++pushing;
            struct Pushing { // leaves with the lock held, whatever status() did to it
                StageQueue *q;
                std::unique_lock<std::mutex> &lk;
                ~Pushing()
                {
                    if (!lk.owns_lock()) lk.lock();
                    --q->pushing;
                }
            } guard{this, lk};
            for (;;) {
                if (const int rc = status(lk)) return rc;
                if (staged_records == 0 || staged_records + n_records <= max_staged) break;
                const auto t0 = std::chrono::steady_clock::now();
                cv_space.wait(lk);
                blocked_us += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
            }
            std::unique_ptr<Batch> nb(new Batch());
            nb->ticket = next_ticket;
            nb->n_records = n_records;
            nb->rec_base = total_records;
            b = nb.get();
            queue.push_back(std::move(nb));
            try {
                init(*b);
            } catch (...) {
                queue.pop_back();
                throw;
            }
            if (bytes) b->mem = pool.take(bytes);
            ++next_ticket;
            total_records += n_records;
            staged_records += n_records;
            ++pushing; // (the copy below: until the batch is ready)
        }
        // outside the lock: the allocation, where the pool had none, and the copy.  The batch stays in the queue until it
        // is ready (the worker waits for that), so `b` is valid.
        if (bytes && !b->mem.p) {
            const size_t cap = bytes + bytes / 8 + 4096; // (batches of a run are of one size, more or less)
            if (alloc(cap, &b->mem)) {
                b->mem.bytes = cap;
            } else {
                b->mem = StageMem();
                b->unstaged = true;
            }
        }
        if (b->mem.p) fill((char *)b->mem.p);
        const uint64_t ticket = b->ticket;
        const bool unstaged = b->unstaged;
        {
            std::lock_guard<std::mutex> lk(mu);
            b->ready = true;
            --pushing;
        }
        cv_work.notify_all();
        if (unstaged) return kStageNoMemory;
        if (out_ticket) *out_ticket = ticket;
        return 0;
    }

    int pushes_in_flight() const
    {
        std::lock_guard<std::mutex> lk(mu);
        return pushing;
    }
    // the owner's status has changed: the waiting pushes ask again
    void wake_pushers() { cv_space.notify_all(); }

    void close()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv_work.notify_all();
        cv_space.notify_all();
        if (worker.joinable()) worker.join();
    }
    void cancel()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            cancelled = true;
        }
        close();
    }

    template <typename Process>
    void work(Process &process)
    {
        for (;;) {
            std::unique_ptr<Batch> b;
            bool skip;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_work.wait(lk, [&] { return (!queue.empty() && queue.front()->ready) || (stop && queue.empty()); });
                if (queue.empty()) break;
                b = std::move(queue.front());
                queue.pop_front();
                skip = cancelled || b->unstaged;
            }
            process(*b, skip);
            {
                std::lock_guard<std::mutex> lk(mu);
                staged_records -= b->n_records;
                pool.give(b->mem);
            }
            cv_space.notify_all();
        }
    }
};

} // namespace oem
