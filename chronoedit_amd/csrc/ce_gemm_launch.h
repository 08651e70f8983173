// Host helpers of the GEMM launchers that need the HIP runtime: the epilogue dispatch and the once-per-device shared-memory attribute.
#pragma once
#include <type_traits>

#include "ce_common.h"

// Calls launch(std::integral_constant<int, E>{}) for the E of EPIS... that equals the run-time `epilogue` and returns its result; CE_ERR_ARG
// when the launcher does not take that epilogue.  The lambda reads its epilogue as `constexpr int E = decltype(e)::value`.
// (A LEFT fold: the compiler instantiates the lambda - and the kernels it names - in the order of the list, a right fold in reverse.)
template <int... EPIS, typename Launch>
inline int ce_dispatch_epilogue(int epilogue, Launch&& launch) {
  int rc = CE_ERR_ARG;
  (void)(... || (epilogue == EPIS && (rc = launch(std::integral_constant<int, EPIS>{}), true)));
  return rc;
}

// hipFuncAttributeMaxDynamicSharedMemorySize = bytes on every kernel given (each one is tried); false when any call failed.
template <typename... Kernel>
inline bool ce_raise_dynamic_lds(int bytes, Kernel*... kernel) {
  bool ok = true;
  ((ok &= hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess), ...);
  return ok;
}

// Runs set() - the attribute calls of one launch site - until it has returned true once on the current device (hipFuncSetAttribute applies
// to the current device only); false while it has not.  The flags belong to the TYPE of the lambda: one set per call site and, inside a
// generic lambda or a template, per instantiation of it.
template <typename Set>
inline bool ce_once_per_device(Set&& set) {
  static bool done_[CE_MAX_DEVICES] = {};
  bool& done = done_[ce_device_slot()];
  if (!done) done = set();
  return done;
}
