// Streaming CheapTrick / mel-cepstrum analysis (wana_stream_kernels.hip): what a stream keeps on
// the device between pushes, the record a push's plan hands its frame kernels, and the sticky flags.
#pragma once
#include "wana_frame.h"

#define WS_THREADS 256
#define WS_HIST 256             // raw fp32 samples kept beside the ring, by absolute position & 255 (the filter needs 254)
#define WS_REACH WA_MAX_HALF    // the furthest a window reaches either side of its origin
#define WS_MAX_QUEUE 65536

#define WS_FLAG_RING 1     // a frame's window start had left the ring: the frame was dropped
#define WS_FLAG_QUEUE 2    // the F0 queue overflowed: the newest rows were dropped
#define WS_FLAG_DRAWS 4    // a draw offset passed the reserved randn table (the kernel's clamp applied)
#define WS_FLAG_PAST_END 8 // at an end push: rows past what the offline call takes, or rows with no sample
#define WS_FLAG_F0 16      // an F0 row not finite, negative or above fs / 4: analysed as unvoiced

struct WsState {
  long long n, rows, emitted;  // samples received, F0 rows received, frames that have left, in the current utterance
  long long doff;              // the randn draw offset of the next frame
  int flags, pad;
};

struct WsPlan {
  long long n_len;  // the stream's length at this push: windows clamp to n_len - 1
  int n_emit, pad;
};

struct WsSlot {  // an emitted frame
  double f0;
  long long index, doff;
};

struct WsGeom {
  int fs, n_taps, ring_n, ring_cap, qcap, m1, first;
  double shiftms, shift;  // shift = shiftms / 1000 * fs, as WorldAnalyzer._batch forms it
  WsState* state;         // [S]
  double* ring;           // [S][ring_n]: the analysed signal by absolute position & (ring_n - 1)
  float* hist;            // [S][WS_HIST]
  double* queue;          // [S][qcap]: F0 row k at k % qcap
  const double* taps;     // [n_taps]; n_taps = 0: no low cut
  WsPlan* plan;           // [S]
  WsSlot* slots;          // [S][qcap]
  double* cep;            // [S][qcap][W_K]: the liftered cepstra of a push's frames
};
