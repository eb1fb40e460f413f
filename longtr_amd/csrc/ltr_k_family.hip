// ltr_k_family.hip -- the family kernel (ltr_dp_family.hpp): the pairs of one read against several haplotypes of its locus, the
// rows their windows share scored once; members the acceptance rule or a certificate does not clear scored in line by the exact
// bodies (ltr_dp_redo.hpp).  Symmetric indel models only (the 11-operation cell): the host forms no family otherwise.
#include <hip/hip_runtime.h>

#include "ltr_kernels.h"

namespace {
#include "ltr_dp_kernel.hpp"
#include "ltr_dp_redo.hpp"
typedef __attribute__((address_space(4))) const FamilyArgs* FamArgPtr;
#include "ltr_dp_family.hpp"
}  // namespace

namespace ltrk {
hipError_t occ_family(int* per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, ltr_dp_family_kernel, 64 * kBlockWaves, 0);
}
void launch_family(dim3 grid, hipStream_t st, const KernelArgs& A, const FamilyArgs& F) {
  hipLaunchKernelGGL(ltr_dp_family_kernel, grid, dim3(64 * kBlockWaves), 0, st, A, F);
}
}  // namespace ltrk
