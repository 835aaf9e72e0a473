// Device-resident FIFOs of km_legacy_stream_* -- the reference's RingBuffer (scripts/rt_simplified.py:46-97) for every stream at
// once.  A stream owns lfifo_len samples and three integers (write_ptr, read_ptr, available) in Context::lfifo_state.
//
//   fifo_push_kernel   RingBuffer.write (:56-77): stream s appends min(count[s], lfifo_len - available[s]) samples at its write
//                      pointer, with wrap-around, and drops the rest.
//   fifo_pop_kernel    RingBuffer.read(audio_length) (:79-97): ready[s] = available[s] >= audio_length; a ready stream's window
//                      is copied in chronological order into the dense staging image (streams, audio_length) that the plain
//                      front end reads, and its read pointer and count advance.  A stream that is not ready moves nothing.
//
// One workgroup per stream in both: the workgroup reads the stream's state, copies, and one thread writes the new state behind a
// barrier -- plain stores, no atomics, nothing read back by the host.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_context.h"

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (void)hipGetLastError();                                                          \
            return km::fail(KM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));              \
        }                                                                                     \
    } while (0)

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

int launch_lfifo_push(Context* c, const float* samples, int64_t n_per_stream, const int* counts, void* stream) {
    hipLaunchKernelGGL(fifo_push_kernel, dim3((unsigned)c->lfifo_streams), dim3(kFifoPushThreads), 0, (hipStream_t)stream, c->lfifo,
                       c->lfifo_state, (int)c->lfifo_streams, (int)c->lfifo_len, samples, (int)n_per_stream, counts);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int launch_lfifo_pop(Context* c, unsigned char* ready_out, void* stream) {
    hipLaunchKernelGGL(fifo_pop_kernel, dim3((unsigned)c->lfifo_streams), dim3(kFifoPopThreads), 0, (hipStream_t)stream, c->lfifo,
                       c->lfifo_state, (int)c->lfifo_streams, (int)c->lfifo_len, (int)c->lfifo_window, c->lfifo_stage, c->lfifo_ready,
                       ready_out);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // namespace km
