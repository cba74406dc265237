/* sao_types.h -- the per-CTB operands of sample adaptive offset as the kernels read them.  Plain data, no HIP: included by the
 * launch interface (deblock_kernels.h) and by sao_packed.h, which tests/sao_sim compiles for the CPU. */
#pragma once
#include <stdint.h>

struct DbkSaoCtb {
    uint8_t type;     /* 0 off, 1 band, 2 edge */
    uint8_t cls;      /* band position / edge class */
    int8_t offset[4]; /* SaoOffsetVal[1..4] */
};

/* slice / tile boundaries SAO must not look across (H.265 8.7.3.2; hevcdbk_sao_borders of the C ABI): one byte per CTB of the
 * plane's own CTB grid, HEVCDBK_SAO_NOX_* bits.  A kernel argument of its own, taken by the _nox kernels only: the kernels
 * without the operand keep their argument layout, i.e. their machine code */
struct DbkSaoNox {
    const uint8_t *nox;
    int stride;
    long long frame_stride; /* bytes, 0 = shared */
};
