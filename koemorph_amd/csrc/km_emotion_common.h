// What the emotion streams (km_emotion_stream.hip) and the emotion track of a clip (km_emotion_clip.hip) share: the sizes of the two
// back ends, the timing law of the reference's OpenSMILEeGeMAPSExtractor in samples with its refusals, the scrub and frame count of
// a window, and the carving of an object's one allocation.  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_context.h"

namespace km {

namespace emo {
constexpr int SR = 16000, NFEAT = 88, NEMO = 256, REC = 36, MAXF = 2048;   // NFEAT: eGeMAPS; a GeMAPS object has egm::NFEAT_GEMAPS = 62 (km_egemaps_dev.h)
constexpr int NBASIC = 9, BASIC_REC = 4, BASIC_HOP = 512, BASIC_MAX_WINDOW = 1 << 20;   // the `basic` back end (km_prosody.hip)
}  // namespace emo

__device__ __forceinline__ float emo_scrub(float f) { return fabsf(f) <= 3.4028234663852886e38f ? f : 0.f; }    // NaN, +Inf, -Inf -> 0 (np.nan_to_num, :450-452)

__device__ __forceinline__ int emo_slot_frames(int len) { return (len - 960) / 160 + 1; }    // km_egemaps_num_frames; len >= min_samples = 8000

// The ring of context + 2 s (opensmile_extractor.py:245-248), the window get_window(context) returns once that much has arrived, the
// samples between two updates, the half second below which nothing is extracted (:388-389), the frame records of a full window.
struct EmoTiming {
    int ring_len = 0, window_len = 0, update_samples = 0, min_samples = 0, max_nf = 0;
};

// The reference constructor's own checks (:204-209).  An object's checks of its counts come between these and emo_timing: that is
// the order in which the refusals win.  `fn` is the name the texts carry.
inline int emo_check_seconds(const char* fn, double context_window_s, double update_interval_s) {
    if (!(context_window_s >= 1.0)) return fail(KM_ERR_INVALID_ARG, "%s: Context window must be at least 1.0 seconds", fn);
    if (!(update_interval_s >= 0.1)) return fail(KM_ERR_INVALID_ARG, "%s: Update interval must be at least 0.1 seconds", fn);
    if (update_interval_s > context_window_s) return fail(KM_ERR_INVALID_ARG, "%s: Update interval cannot be larger than context window", fn);
    return KM_OK;
}

// The law in samples for checked seconds, or the refusal of what the kernels of the back end cannot hold.  long_windows (eGeMAPS
// only, km_emotion_*_create_long): the window limit of the basic back end takes the place of the 2048 frames.
inline int emo_timing(const char* fn, double context_window_s, double update_interval_s, bool basic, EmoTiming* t, bool long_windows = false) {
    using namespace emo;
    if (context_window_s > 3600.0) return fail(KM_ERR_UNSUPPORTED, "%s: context window of %g s", fn, context_window_s);
    const int64_t R = (int64_t)((context_window_s + 2.0) * SR), Cw = (int64_t)(context_window_s * SR), C = Cw < R ? Cw : R;
    const int64_t nf = basic ? 1 + C / BASIC_HOP : km_egemaps_num_frames(C);          // 32 ms or 10 ms frames
    if ((basic || long_windows) && C > BASIC_MAX_WINDOW)
        return fail(KM_ERR_UNSUPPORTED, "%s: a window of %lld samples, at most %d (65.5 s)", fn, (long long)C, BASIC_MAX_WINDOW);
    if (!basic && !long_windows && nf > MAXF) return fail(KM_ERR_UNSUPPORTED, "%s: %lld frames per window, at most %d (20.5 s)", fn, (long long)nf, MAXF);
    t->ring_len = (int)R; t->window_len = (int)C; t->update_samples = (int)(update_interval_s * SR); t->min_samples = SR / 2; t->max_nf = (int)nf;
    return KM_OK;
}

// One allocation, carved into 16-byte aligned pieces: lay the object out once over a null base to learn the size (`at`), then over
// the allocation.
struct EmoCarver {
    char* base;
    int64_t at = 0;
    template <class T>
    T* take(int64_t count) {
        T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += (count * (int64_t)sizeof(T) + 15) / 16 * 16;
        return p;
    }
};

}  // namespace km
