// Formulation A wavefront-per-QP kernels, 3 ZMP rows per lane (C <= 192), in the form that also stores the whole decision of every QP
// (ismpc_a_tick_wave<Horizon<Real>, ...>: ismpc_a_tick_batch_horizon_device).  A unit of its own, so that these instantiations compile
// beside the plain ones of ismpc_a_wave_rl3.hip and not behind them.
#include "ismpc_a_wave.hpp"
namespace ismpc_a { int launch_wave_rl3_hz(const WaveLaunch& L, hipError_t* err) { return launch_wave_horizon<3>(L, err); } }
