// qkv_attn_fused_body.inc -- the statements of the fused q | k | v + attention kernel (gemv_q80_impl.h), included textually into its two
// forms: qkv_attn_fused_kernel<NV, UPW> (the projection's rows fold through the LDS product table) and qkv_attn_fused_wf_kernel (rows of one chunk,
// n == 1024: every wave folds its own rows, gemv_q80_slab_body.inc SLAB_WF; NV = UPW = 1).  The includer defines SLAB_WF; fa, NV, UPW are in scope.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint2 tk_ = hand_tick(fa.hand);                       // the step's epoch: the first load of every workgroup
    if (blockIdx.x >= fa.ngemv) {
        const uint32_t ab = blockIdx.x - fa.ngemv;
        const uint32_t split = ab / fa.head_wgs, grp = ab - split * fa.head_wgs;
        attention_body<8, 4, 1, 1, false, false, 2, false, true>(fa.a, smem, grp, 0u, split, fa.hand, hand_ctag(tk_, fa.hand), fa.wait16);
        return;
    }
    constexpr int ROLE = R_NORM_STORE, GS = 64, B = 1;
#define SLAB_A fa.g
#define SLAB_BID blockIdx.x
#define SLAB_HAND 1
#define SLAB_HANDV fa.hand
#define SLAB_PTAG hand_ptag(tk_, fa.hand)
#define SLAB_XHAND 0
#define SLAB_XHANDV (SlabHand{})
#define SLAB_CTAG 0u
#define SLAB_PART 0
#include "gemv_q80_slab_body.inc"
#undef SLAB_A
#undef SLAB_BID
#undef SLAB_HAND
#undef SLAB_HANDV
#undef SLAB_PTAG
#undef SLAB_XHAND
#undef SLAB_XHANDV
#undef SLAB_CTAG
#undef SLAB_PART
