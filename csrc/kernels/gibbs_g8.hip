// Instantiations of the Gibbs sweep kernels for 8- and 16-lane units (K > 112, ONI_TILING=narrow) (see gibbs_sampler.h).
#include "gibbs_sampler.h"

int oni_gibbs_dispatch_g8(const OniGibbs& a, int G, int KP, bool init, int mode, int qpf, hipStream_t s, int* which) {
#define ONI_GIBBS_CASE(g_, kp_) \
  if (G == g_ && KP == kp_) return launch_gibbs<g_, kp_>(a, init, mode, qpf, s, which);
  ONI_TILINGS_G8(ONI_GIBBS_CASE)
  ONI_TILINGS_G16(ONI_GIBBS_CASE)
#undef ONI_GIBBS_CASE
  return (int)hipErrorInvalidValue;
}
