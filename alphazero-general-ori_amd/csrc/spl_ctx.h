// spl_ctx.h — the context behind include/splendor_amd.h's opaque spl_ctx, for every
// translation unit of the library (created and changed in splendor_env.hip only).
#pragma once

struct spl_ctx {
    int n;              // players, 2..4
    int token_limit;
    int rules;          // SPL_RULE_* flags
};

inline bool ok_ctx(const spl_ctx *c) { return c && c->n >= 2 && c->n <= 4; }
