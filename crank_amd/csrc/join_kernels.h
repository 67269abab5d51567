// The frame join's per-stream state and the plan of one push (join_kernels.hip).  The plan is a
// pure function of the old state and the push's counts: both kernels of a push derive it from the same old state, and
// tests/join_ref.py restates it.
#pragma once

// One side's ring has cap + max_in SLOTS for at most cap waiting rows: waiting row i sits in slot (head + i) % slots.
struct JoinSide {
  int width, max_in, cap, slots;
};

struct JoinState {
  int wait_a, wait_b;  // waiting rows
  int head_a, head_b;  // slot of the oldest waiting row
  int first;           // pairs emitted so far in this utterance
  int overflow;        // sticky: bit 0 ring A, bit 1 ring B lost rows
  int pad[2];
};

struct JoinPlan {
  int a0, b0, na, nb, take, end;
  int keep_a, keep_b;  // new rows of each side that enter its ring: rows [skip, skip + keep) of the push's input
  int skip_a, skip_b;  // new rows taken by this push's pairs
  int lost_a, lost_b;  // new rows that found no room (never with end)
  int dropped;         // with end: the surplus that is discarded
};

__host__ __device__ inline int join_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// What one side keeps: w0 rows wait, n arrive, take leave; with end nothing stays.
__host__ __device__ inline void join_side_plan(int w0, int n, int take, int cap, int end, int& skip, int& keep, int& lost) {
  skip = take > w0 ? take - w0 : 0;            // new rows that leave at once
  const int old_left = w0 > take ? w0 - take : 0;
  const int surplus = n - skip, room = cap - old_left;  // (old_left <= w0 <= cap)
  keep = end ? 0 : (surplus < room ? surplus : room);
  lost = end ? 0 : surplus - keep;
}

__host__ __device__ inline JoinPlan join_plan(const JoinState& st, const JoinSide& A, const JoinSide& B, int n_a, int n_b,
                                              int end) {
  JoinPlan p;
  p.a0 = st.wait_a; p.b0 = st.wait_b;
  p.na = join_clamp(n_a, A.max_in); p.nb = join_clamp(n_b, B.max_in);
  p.end = end != 0;
  const int ta = p.a0 + p.na, tb = p.b0 + p.nb;
  p.take = ta < tb ? ta : tb;
  join_side_plan(p.a0, p.na, p.take, A.cap, p.end, p.skip_a, p.keep_a, p.lost_a);
  join_side_plan(p.b0, p.nb, p.take, B.cap, p.end, p.skip_b, p.keep_b, p.lost_b);
  p.dropped = p.end ? (ta - p.take) + (tb - p.take) : 0;
  return p;
}

__host__ __device__ inline JoinState join_next(const JoinState& st, const JoinSide& A, const JoinSide& B, const JoinPlan& p) {
  JoinState n = st;
  if (p.end) {
    n.wait_a = n.wait_b = n.head_a = n.head_b = n.first = 0;  // (the overflow flags stay: they are sticky until a reset)
    return n;
  }
  n.wait_a = p.a0 + p.na - p.take - p.lost_a;
  n.wait_b = p.b0 + p.nb - p.take - p.lost_b;
  n.head_a = A.slots ? (st.head_a + p.take) % A.slots : 0;
  n.head_b = B.slots ? (st.head_b + p.take) % B.slots : 0;
  n.first = st.first + p.take;
  n.overflow = st.overflow | (p.lost_a ? 1 : 0) | (p.lost_b ? 2 : 0);
  return n;
}
