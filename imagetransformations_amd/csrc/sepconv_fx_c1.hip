// The FIXED (8-bit fixed-point taps, round half up) sepconv kernels for C=1 interleaved channels: every instantiation
// launch_sepconv (sepconv_launch.inc) can reach for a plan of sepconv_route.h.
#include "sepconv_launch.inc"
template int imgxf::launch_sepconv<1, true>(const SepconvPlan&, const View&, const View&, const View&, const Taps&, hipStream_t);
