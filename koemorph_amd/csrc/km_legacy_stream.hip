// Device-resident FIFOs of km_legacy_stream_* -- the reference's RingBuffer (scripts/rt_simplified.py:46-97) for every stream at
// once.  A stream owns lf.len samples and three integers (write_ptr, read_ptr, available) in Context::lf.state.
//
//   fifo_push_kernel   RingBuffer.write (:56-77): stream s appends min(count[s], lf.len - available[s]) samples at its write
//                      pointer, with wrap-around, and drops the rest.
//   fifo_pop_kernel    RingBuffer.read(audio_length) (:79-97): ready[s] = available[s] >= audio_length; a ready stream's window
//                      is copied in chronological order into the dense staging image (streams, audio_length) that the plain
//                      front end reads, and its read pointer and count advance.  A stream that is not ready moves nothing.
//
// One workgroup per stream in both: the workgroup reads the stream's state, copies, and one thread writes the new state behind a
// barrier -- plain stores, no atomics, nothing read back by the host.
//
// The chunk FIFOs of km_stream_feed / _step (the production model's loop, scripts/rt.py:48-99, 343-372) have the same layout in
// Context::st.fifo and share fifo_push_kernel.  Their pop has no staging image, because the destination is the stream's ring:
//
//   fifo_pop_ring_kernel         RingBuffer.read(frame) + MelAudioBuffer.add_audio_frame (mel_sliding_window.py:70-116) for every
//                                stream that holds a frame; fire[s] = popped && is_full is the gate of the step's other kernels.
//   stream_reset_masked_kernel   MelSlidingWindowExtractor.reset (:373-383) + reset_temporal_state for the streams of a mask.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_context.h"


namespace km {

constexpr int kFifoPushThreads = 256, kFifoPopThreads = 1024;

__global__ __launch_bounds__(kFifoPushThreads) void fifo_push_kernel(float* __restrict__ fifo, int* __restrict__ state, int n_streams,
                                                                     int len, const float* __restrict__ samples, int n_in,
                                                                     const int* __restrict__ counts) {
    const int s = blockIdx.x;
    const int w0 = state[s], avail = state[2 * n_streams + s];
    int cnt = counts ? counts[s] : n_in;
    cnt = cnt < 0 ? 0 : (cnt > n_in ? n_in : cnt);
    const int n = cnt < len - avail ? cnt : len - avail;          // what does not fit is dropped (:58-61)
    float* r = fifo + (int64_t)s * len;
    const float* in = samples + (int64_t)s * n_in;
    for (int i = threadIdx.x; i < n; i += kFifoPushThreads) {
        int p = w0 + i;
        p -= p >= len ? len : 0;
        r[p] = in[i];
    }
    __syncthreads();                                              // every thread has read the state
    if (threadIdx.x == 0 && n > 0) {
        int w = w0 + n;
        w -= w >= len ? len : 0;
        state[s] = w;
        state[2 * n_streams + s] = avail + n;
    }
}

__global__ __launch_bounds__(kFifoPopThreads) void fifo_pop_kernel(const float* __restrict__ fifo, int* __restrict__ state, int n_streams,
                                                                   int len, int window, float* __restrict__ stage,
                                                                   unsigned char* __restrict__ ready, unsigned char* __restrict__ ready_out) {
    const int s = blockIdx.x;
    const int r0 = state[n_streams + s], avail = state[2 * n_streams + s];
    const bool ok = avail >= window;                              // :81-82
    if (threadIdx.x == 0) {
        ready[s] = ok ? 1 : 0;
        if (ready_out) ready_out[s] = ok ? 1 : 0;
    }
    if (!ok) return;                                              // uniform over the workgroup
    const float* r = fifo + (int64_t)s * len;
    float* dst = stage + (int64_t)s * window;
    if (((r0 | len | window) & 3) == 0) {
        // 16-byte accesses: the read pointer, the ring and the window are whole float4s, so none straddles the wrap and the
        // stream's staging row begins on a 16-byte boundary
        const int n4 = window >> 2, r4 = r0 >> 2, len4 = len >> 2;
        const float4* src4 = reinterpret_cast<const float4*>(r);
        float4* dst4 = reinterpret_cast<float4*>(dst);
        for (int i = threadIdx.x; i < n4; i += kFifoPopThreads) {
            int p = r4 + i;
            p -= p >= len4 ? len4 : 0;
            dst4[i] = src4[p];
        }
    } else {
        for (int i = threadIdx.x; i < window; i += kFifoPopThreads) {
            int p = r0 + i;
            p -= p >= len ? len : 0;
            dst[i] = r[p];
        }
    }
    __syncthreads();                                              // every thread has read the state
    if (threadIdx.x == 0) {
        int rn = r0 + window;
        rn -= rn >= len ? len : 0;
        state[n_streams + s] = rn;
        state[2 * n_streams + s] = avail - window;
    }
}

// RingBuffer.read(frame) (rt.py:79-99) + MelAudioBuffer.add_audio_frame (mel_sliding_window.py:70-116), one workgroup per stream.  A
// stream holding fewer than `frame` samples writes fire[s] = 0 (and its unchanged is_full / backlog) and returns: a uniform exit
// ahead of the barrier.  Otherwise min(frame, hop) samples go from the FIFO at its read pointer (modular) into the ring at its
// write pointer (modular), zeros behind them when frame < hop (:84-89; a longer frame loses its tail, :90-91: 533 -> 532 at
// 30 fps), and behind the barrier thread 0 stores the FIFO state, the ring state and the flags.  No LDS: every sample is one
// coalesced load and one coalesced store, 1 KB a wave.  is_full follows :112 and never falls back to 0.
__global__ __launch_bounds__(kFifoPushThreads) void fifo_pop_ring_kernel(const float* __restrict__ fifo, int* __restrict__ state, int n_streams,
                                                                         int len, int frame, float* __restrict__ ring, int* __restrict__ wptr,
                                                                         int* __restrict__ frames, unsigned char* __restrict__ ready, int hop,
                                                                         int ring_len, unsigned char* __restrict__ fire,
                                                                         unsigned char* __restrict__ fire_out, unsigned char* __restrict__ ready_out,
                                                                         int* __restrict__ backlog) {
    const int s = blockIdx.x;
    const int r0 = state[n_streams + s], avail = state[2 * n_streams + s];
    if (avail < frame) {                                          // rt.py:81-82; uniform over the workgroup
        if (threadIdx.x == 0) {
            fire[s] = 0;
            if (fire_out) fire_out[s] = 0;
            if (ready_out) ready_out[s] = ready[s];
            if (backlog) backlog[s] = 0;                          // avail / frame
        }
        return;
    }
    const int w0 = wptr[s];
    const float* f = fifo + (int64_t)s * len;
    float* r = ring + (int64_t)s * ring_len;
    const int ncopy = frame < hop ? frame : hop;
    for (int i = threadIdx.x; i < hop; i += kFifoPushThreads) {
        int q = r0 + i;
        q -= q >= len ? len : 0;
        int p = w0 + i;
        p -= p >= ring_len ? ring_len : 0;
        r[p] = i < ncopy ? f[q] : 0.f;
    }
    __syncthreads();                                              // every thread has read the state
    if (threadIdx.x == 0) {
        int rn = r0 + frame;
        rn -= rn >= len ? len : 0;
        state[n_streams + s] = rn;
        state[2 * n_streams + s] = avail - frame;
        int w = w0 + hop;
        w -= w >= ring_len ? ring_len : 0;
        wptr[s] = w;
        const int n = frames[s] + 1;
        frames[s] = n;
        const unsigned char full = (ready[s] || (int64_t)n * hop >= ring_len) ? 1 : 0;
        ready[s] = full;
        fire[s] = full;
        if (fire_out) fire_out[s] = full;
        if (ready_out) ready_out[s] = full;
        if (backlog) backlog[s] = (avail - frame) / frame;
    }
}

// The streams with mask[s] != 0 become what km_stream_create left: FIFO pointers (when there are FIFOs), ring write pointer, frame
// count, is_full, started and the EMA state all zero.  The samples of the ring and the FIFO stay: neither is read before it is
// written again.  A FIFO sample is read only below `available`, i.e. after a write put it there; the ring is read only while
// is_full, which takes frames * hop >= ring_len pushes of hop consecutive samples from write pointer 0 -- every sample of it.
__global__ __launch_bounds__(64) void stream_reset_masked_kernel(const unsigned char* __restrict__ mask, int n_streams, int* __restrict__ fifo_state,
                                                                 int* __restrict__ wptr, int* __restrict__ frames, unsigned char* __restrict__ ready,
                                                                 unsigned char* __restrict__ started, unsigned char* __restrict__ fire,
                                                                 float* __restrict__ ema, int nb) {
    const int s = blockIdx.x;
    if (!mask[s]) return;                                         // uniform over the workgroup
    for (int i = threadIdx.x; i < nb; i += 64) ema[(int64_t)s * nb + i] = 0.f;
    if (threadIdx.x == 0) {
        if (fifo_state) {
            fifo_state[s] = 0; fifo_state[n_streams + s] = 0; fifo_state[2 * n_streams + s] = 0;
            fire[s] = 0;
        }
        wptr[s] = 0; frames[s] = 0; ready[s] = 0; started[s] = 0;
    }
}

int launch_lfifo_push(Context* c, const float* samples, int64_t n_per_stream, const int* counts, void* stream) {
    hipLaunchKernelGGL(fifo_push_kernel, dim3((unsigned)c->lf.streams), dim3(kFifoPushThreads), 0, (hipStream_t)stream, c->lf.fifo,
                       c->lf.state, (int)c->lf.streams, (int)c->lf.len, samples, (int)n_per_stream, counts);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int launch_lfifo_pop(Context* c, unsigned char* ready_out, void* stream) {
    hipLaunchKernelGGL(fifo_pop_kernel, dim3((unsigned)c->lf.streams), dim3(kFifoPopThreads), 0, (hipStream_t)stream, c->lf.fifo,
                       c->lf.state, (int)c->lf.streams, (int)c->lf.len, (int)c->lf.window, c->lf.stage, c->lf.ready,
                       ready_out);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int launch_sfifo_push(Context* c, const float* samples, int64_t n_per_stream, const int* counts, void* stream) {
    hipLaunchKernelGGL(fifo_push_kernel, dim3((unsigned)c->st.n_streams), dim3(kFifoPushThreads), 0, (hipStream_t)stream, c->st.fifo.samples,
                       c->st.fifo.state, (int)c->st.n_streams, (int)c->st.fifo.len, samples, (int)n_per_stream, counts);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int launch_sfifo_pop_ring(Context* c, unsigned char* fire_out, unsigned char* ready_out, int* backlog_out, void* stream) {
    hipLaunchKernelGGL(fifo_pop_ring_kernel, dim3((unsigned)c->st.n_streams), dim3(kFifoPushThreads), 0, (hipStream_t)stream, c->st.fifo.samples,
                       c->st.fifo.state, (int)c->st.n_streams, (int)c->st.fifo.len, c->st.fifo.frame, c->st.ring, c->st.ring_wptr, c->st.ring_frames,
                       c->st.ring_ready, c->st.ring_hop, (int)c->st.ring_len, c->st.fifo.fire, fire_out, ready_out, backlog_out);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int launch_stream_reset_masked(Context* c, const unsigned char* mask, void* stream) {
    hipLaunchKernelGGL(stream_reset_masked_kernel, dim3((unsigned)c->st.n_streams), dim3(64), 0, (hipStream_t)stream, mask, (int)c->st.n_streams,
                       c->st.fifo.len > 0 ? c->st.fifo.state : nullptr, c->st.ring_wptr, c->st.ring_frames, c->st.ring_ready, c->st.ring_started,
                       c->st.fifo.fire, c->st.ring_state, c->NB);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // namespace km
