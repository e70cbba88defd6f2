// Who owns which of an encode slot's two hand-off sets.  A hand-off set is what an encode call still uses after it has given
// its slot to the next call ("queue ahead", encode_batch_impl in api.cpp: timing events, the pinned landing buffer, a packed-
// archive buffer and its events -- HandoffSet there).  This header is the rule alone and knows nothing of the device, so that
// tools/handoff_probe.cpp can play it on host threads under a thread sanitizer.
//
// The rule: a call that has taken the slot takes set `counter++ & 1` (take) and waits there until the call two before it has
// released that set; it keeps the set when it unlocks the slot and releases it once it no longer reads or queues anything
// that names the set (HandoffOwner: on every return path).  A call that keeps the slot over several DEFLATE passes borrows
// the other set for every second pass through the same wait (acquire).  take() and acquire() are for the holder of the slot
// mutex only; release() may come from any thread.  Whoever waits here holds the slot and no share of g_quiesce (host.h), and
// the owner it waits for needs neither.
#pragma once
#include <condition_variable>
#include <mutex>

namespace cct {

class HandoffRing {
	std::mutex m;
	std::condition_variable cv;
	bool owned[2] = {false, false};
	unsigned counter = 0;  // calls that have taken the slot so far (written under the slot mutex)

public:
	unsigned take() { const unsigned k = counter++ & 1u; acquire(k); return k; }
	void acquire(unsigned k)
	{
		std::unique_lock<std::mutex> l(m);
		cv.wait(l, [&] { return !owned[k]; });
		owned[k] = true;
	}
	void release(unsigned k)
	{
		{ std::lock_guard<std::mutex> l(m); owned[k] = false; }
		cv.notify_all();
	}
};

// One set of one ring, owned from construction until release() or the end of the scope, whichever comes first.
class HandoffOwner {
	HandoffRing *ring;
	unsigned k;

public:
	explicit HandoffOwner(HandoffRing &r) : ring(&r), k(r.take()) {}                  // the call's own set
	HandoffOwner(HandoffRing &r, unsigned set) : ring(&r), k(set) { r.acquire(set); }  // a borrowed one
	~HandoffOwner() { release(); }
	HandoffOwner(const HandoffOwner &) = delete;
	HandoffOwner &operator=(const HandoffOwner &) = delete;
	unsigned set() const { return k; }
	void release() { if (ring) ring->release(k); ring = nullptr; }
};

}  // namespace cct
