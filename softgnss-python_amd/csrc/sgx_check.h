// What a translation unit of libsgx.so needs to refuse an argument, and nothing of HIP: with this header alone the scalar
// host files (sgx_core.cpp, sgx_geo.cpp, sgx_navhost.cpp) build with a plain C++ compiler too (tools/sanitize_host.sh).
#pragma once
#include "sgx.h"

#define SGX_VERSION_STR "sgx 0.1 (gfx950)"

// The calling thread's error text (sgx_core.cpp), as sgx_last_error hands it out
void sgx_set_error(const char* fmt, ...);

#define SGX_CHECK_ARG(cond)                                                 \
    do {                                                                    \
        if (!(cond)) {                                                      \
            sgx_set_error("bad argument: %s (%s:%d)", #cond, __FILE__, __LINE__); \
            return SGX_E_ARG;                                               \
        }                                                                   \
    } while (0)
