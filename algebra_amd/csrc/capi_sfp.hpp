// What the C ABI units of the one-word fields share: capi_sfp.hip defines these, capi_fri.hip uses them.
#pragma once
#include "capi_core.hpp"
#include "sfp_fft.cuh"
#include "sfp_internal.hpp"

#define ARK_SFP_SWITCH(sfield, CALL)                       \
  switch (sfield) {                                        \
    case ARK_HIP_SFP_GOLDILOCKS: return CALL(GOLDILOCKS);  \
    case ARK_HIP_SFP_BABYBEAR: return CALL(BABYBEAR);      \
    case ARK_HIP_SFP_KOALABEAR: return CALL(KOALABEAR);    \
  }                                                        \
  return ARK_HIP_ERR_ARG

namespace arkhip {
namespace capi {

// what the host code needs of a field, by id
struct SfpHost {
  int bytes, two_adicity;
  uint64_t p, one;
  uint64_t (*mul)(uint64_t, uint64_t);
  uint64_t (*pow)(uint64_t, uint64_t);
  uint64_t (*from_canonical)(uint64_t);
  uint64_t root;
};
// nullptr for an id this build does not serve (the development build serves none)
const SmallFieldOps* sfp_ops(int sfield);
int sfp_host(int sfield, SfpHost* h);
// a domain the transforms accept: the size matches its log and the field can hold it
int domain_check(const SfpHost& h, const ark_hip_sfp_radix2_domain* dom);
// the cached two-level power table of (sfield, k, g, scale): hi | lo in one buffer
int powers_for(Context* c, int sfield, const SfpHost& h, const SmallFieldOps* ops, int k, uint64_t g, uint64_t scale, SfpScale* out);

}  // namespace capi
}  // namespace arkhip
