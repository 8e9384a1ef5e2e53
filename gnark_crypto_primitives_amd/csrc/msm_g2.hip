// G2 half of the batched MSM: the Fq2 instantiations of the table builds and of the launch routines
// of msm_impl.h (msm.hip declares them extern), in an object of their own so that the two halves
// compile in parallel.
#include "msm_impl.h"

namespace zk {

template int build_comb<Fq2>(zkmi_ctx*, const Affine<Fq2>*, size_t, const WinPlan&, int,
                             Affine<Fq2>*, int*, Affine<Fq2>*);
template int build_impl<Fq2>(zkmi_ctx*, const Affine<Fq2>*, size_t, const WinPlan&, Affine<Fq2>*);
template int run_impl<Fq2>(zkmi_ctx*, const zkmi_msm_bases*, const Fr*, const uint32_t*, size_t,
                           size_t, XYZZ<Fq2>*, bool, XYZZ<Fq2>*, hipStream_t, const uint8_t*, bool);

}  // namespace zk
