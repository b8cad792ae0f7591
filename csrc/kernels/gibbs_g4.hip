// Instantiations of the Gibbs sweep kernels for four-lane units (K = 57..112) (see gibbs_sampler.h).
#include "gibbs_sampler.h"

int oni_gibbs_dispatch_g4(const OniGibbs& a, int G, int KP, bool init, int mode, int qpf, hipStream_t s, int* which) {
#define ONI_GIBBS_CASE(g_, kp_) \
  if (G == g_ && KP == kp_) return launch_gibbs<g_, kp_>(a, init, mode, qpf, s, which);
  ONI_TILINGS_G4(ONI_GIBBS_CASE)
#undef ONI_GIBBS_CASE
  return (int)hipErrorInvalidValue;
}
