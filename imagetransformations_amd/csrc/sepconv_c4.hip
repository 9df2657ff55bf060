// The float sepconv kernels for C=4 interleaved channels: every instantiation launch_sepconv (sepconv_launch.inc) can
// reach for a plan of sepconv_route.h.
#include "sepconv_launch.inc"
template int imgxf::launch_sepconv<4, false>(const SepconvPlan&, const View&, const View&, const View&, const Taps&, hipStream_t);
