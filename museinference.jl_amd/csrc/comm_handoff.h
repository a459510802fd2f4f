// comm_handoff.h -- how the RCCL transport's caller thread hands a result area's gather to the communicator's worker thread
// (muse_comm.cpp): a FIFO of areas under a mutex and a condition variable, and one flag per area that tells the caller the
// worker has put the area's collective on its stream.  Host code only, no HIP call in it
// (tests/native/handoff_driver.cpp runs it under ThreadSanitizer).
#pragma once
#include <atomic>
#include <condition_variable>
#include <mutex>

namespace muse {

template <int kAreas>
class AreaHandoff {
  public:
    AreaHandoff() { for (int a = 0; a < kAreas; ++a) enqueued_[a].store(0); }
    // caller: an area is in the queue at most once (its previous gather has been awaited), so the queue never overflows;
    // what the caller wrote before this call is the worker's to read after take() returns the area
    void post(int area) {
        enqueued_[area].store(0, std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> lk(mu_);
            queue_[tail_++ % kAreas] = area;
        }
        cv_.notify_one();
    }
    // worker: the next area, in the order posted; false: stop was requested and nothing is left
    bool take(int& area) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || head_ != tail_; });
        if (head_ == tail_) return false;
        area = queue_[head_++ % kAreas];
        return true;
    }
    void enqueued(int area) { enqueued_[area].store(1, std::memory_order_release); }            // worker: the area's gather is on the stream
    bool is_enqueued(int area) const { return enqueued_[area].load(std::memory_order_acquire) != 0; }   // caller: polls this
    void stop() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
    }

  private:
    std::mutex mu_;
    std::condition_variable cv_;
    int queue_[kAreas] = {0};    // areas whose gather is to be enqueued, FIFO
    int head_ = 0, tail_ = 0;    // monotonically increasing positions (mod kAreas)
    bool stop_ = false;
    std::atomic<int> enqueued_[kAreas];
};

}  // namespace muse
