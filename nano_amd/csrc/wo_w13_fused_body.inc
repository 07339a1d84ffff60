// wo_w13_fused_body.inc -- the statements of the fused Wo + W1|W3 kernels (gemv_q80_impl.h), included TEXTUALLY into each of them
// (textual for the reason gemv_q80_slab_body.inc gives).  The includer has ROLE_A (Wo's role), WF, WFA and fa (the Wo13Args) in scope and defines
//   WO13_CW   0 | 1: Wo's split-attention combine with in-wave weights and live splits only (gemv_q80_slab_body.inc SLAB_CW)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int GS = 64, B = 1, NV = 1, UPW = 1;
    const uint2 tk_ = hand_tick(fa.hand);
    // Order of issue: Wo's loads, W1|W3's loads, Wo's arithmetic, W1|W3's.  (vmcnt counts in order: loads issued BEFORE Wo's would have to
    // land before Wo may use its own -- the first build had W1|W3's in front and Wo waited for the whole 64 MB of Qwen3-4B's two matrices.)
    // Workgroups beyond Wo's grid run Wo's part 1 on rows past the matrix (out-of-range buffer loads: no traffic) and skip its part 2.
    {
        constexpr int ROLE = ROLE_A;
#define SLAB_BID blockIdx.x
#define SLAB_A fa.wo
#define SLAB_HAND 1
#define SLAB_HANDV fa.hand
#define SLAB_PTAG hand_ptag(tk_, fa.hand)
#define SLAB_XHAND 0
#define SLAB_XHANDV (SlabHand{})
#define SLAB_CTAG 0u
#define SLAB_WFC WFA
#define SLAB_CW WO13_CW
#define SLAB_PART 1
#include "gemv_q80_slab_body.inc"
#undef SLAB_PART
        auto wo_rest = [&]() __attribute__((always_inline)) {
#define SLAB_PART 2
#include "gemv_q80_slab_body.inc"
#undef SLAB_PART
        };
#undef SLAB_WFC
#undef SLAB_CW
#undef SLAB_A
#undef SLAB_HAND
#undef SLAB_HANDV
#undef SLAB_PTAG
#undef SLAB_XHAND
#undef SLAB_XHANDV
#undef SLAB_CTAG
        {
            constexpr int ROLE = R_NORM_SWIGLU;
#define SLAB_A fa.w13
#define SLAB_HAND 0
#define SLAB_HANDV (SlabHand{})
#define SLAB_PTAG 0u
#define SLAB_XHAND 1
#define SLAB_XHANDV fa.hand
#define SLAB_CTAG hand_ctag(tk_, fa.hand)
#define SLAB_XHAND_WAIT (blockIdx.x >= fa.wo_wgs ? fa.wait16 : 0u)
#define SLAB_XHAND_NAP 2
#define SLAB_WF WF
#define SLAB_PART 1
#include "gemv_q80_slab_body.inc"
#undef SLAB_PART
            if (blockIdx.x < fa.wo_wgs) wo_rest();
            __syncthreads();                // (LDS is W1|W3's from here)
#define SLAB_PART 2
#include "gemv_q80_slab_body.inc"
#undef SLAB_PART
#undef SLAB_A
#undef SLAB_HAND
#undef SLAB_HANDV
#undef SLAB_PTAG
#undef SLAB_XHAND
#undef SLAB_XHANDV
#undef SLAB_CTAG
#undef SLAB_XHAND_WAIT
#undef SLAB_XHAND_NAP
#undef SLAB_WF
        }
#undef SLAB_BID
    }
