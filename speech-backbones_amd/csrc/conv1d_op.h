// conv1d_op.h -- the handle behind gtts_conv1d_* and its one planning step, shared by conv1d.hip (forward) and conv1d_train.hip (gradients).
#pragma once
#include "../../include/gradtts_abi.h"
#include "conv1d.h"
#include "kernels.h"

struct gtts_conv1d {
    int mode, cin, cout, K, dil, S;
};

// geometry, size checks and instance of one call; pointers are carried, never read
static inline int conv1d_op_plan(const gtts_conv1d *op, gtts::C1Args &a, gtts::C1Inst *inst) {
    using namespace gtts;
    a.cin = op->cin; a.cout = op->cout; a.S = op->S;
    const int r = conv1d_plan(a, op->mode, op->K, op->dil, inst);
    if (r == C1_OK) return GTTS_OK;
    return fail(r == C1_E_SIZE ? GTTS_E_SHAPE : GTTS_E_CONFIG, "conv1d (cin %d, cout %d, k %d, dilation %d, stride %d, Lin %d): %s", op->cin,
                op->cout, op->K, op->dil, op->S, a.Lin, c1_refusal_text(r));
}
