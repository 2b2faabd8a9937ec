// inst_head_bwd.hip -- the head-only backward kernel (leaf_head_bwd.hpp) and the split of the batch its grid follows.
// One of the translation units of libleaf_hip.so; see leaf_inst.hpp.
#include "leaf_head_bwd.hpp"
#include "leaf_inst.hpp"

HeadBwdKernel leaf_inst_head_bwd() { return leaf_head_bwd_kernel; }

void leaf_head_bwd_plan(int B, int F, int cus, int* S, int* L) {
    const HeadPlan hp = head_plan(B, F, cus);
    *S = hp.S;
    *L = hp.L;
}

unsigned leaf_layout_head_bwd() { return leaf_params_layout(); }                 // the launch structs' layout this unit was compiled with (leaf_inst.hpp)
