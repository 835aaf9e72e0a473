// Guards shared by the C-ABI entry files (km_api*.hip).  Internal: not part of the public ABI.
#pragma once

#include <cstdint>

#include "km_context.h"
#include "km_device.h"

namespace km {

LogParams plan_log_params(MelPlan* p);

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int need_ready(Context* c) {
    if (!c) return fail(KM_ERR_INVALID_ARG, "NULL handle");
    if (!c->dev_finalized) return fail(KM_ERR_NOT_FINALIZED, "call km_finalize after loading the state dict");
    return KM_OK;
}

inline int need_dual(Context* c) {
    if (int rc = need_ready(c)) return rc;
    if (c->kind != 0) return fail(KM_ERR_INVALID_ARG, "this entry point needs a dual-stream handle (km_create), not a legacy one");
    return KM_OK;
}

// The fused core's attention-map output exists for the plain fp32 instantiations only: refused before anything is launched
inline int attn_refused(Context* c, const char* who) {
    if (c->fused_ok && (c->opt.core_split == 3 || c->opt.core_split == 6))
        return fail(KM_ERR_UNSUPPORTED, "%s: the split-bf16 core (core_split %d) has no attention-map output", who, c->opt.core_split);
    return KM_OK;
}

}  // namespace km
