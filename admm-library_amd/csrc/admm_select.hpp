// admm_select.hpp -- run-time flags -> template arguments: the whole mechanism by which a launcher picks one kernel form.
//
//   with_flags([&](auto RS, auto RX) { hipLaunchKernelGGL((kernel<NX, NU, RS(), RX()>), ...); }, resid, relax);
//
// calls the generic lambda with one std::true_type / std::false_type per bool, in order, so a kernel's argument list is
// written once.  The lambda is instantiated for EVERY combination of its flags: which forms get compiled is decided in it,
// by folding a flag away (constexpr bool SC = VF() && SOC();) or by `if constexpr` on the constants.  A pointer only some
// forms read is chosen at the call (SEG() ? l.Omd : nullptr).  Inside a nested lambda, name a flag through a constexpr
// local of the enclosing one (constexpr bool RS = rs();), which needs no capture.
#pragma once

#include <type_traits>

namespace admm {

template <class F>
inline void with_flags(F&& f) { f(); }
template <class F, class... Rest>
inline void with_flags(F&& f, bool b, Rest... rest) {
  if (b) with_flags([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
  else   with_flags([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

// Small integers: f(std::integral_constant<int, K>) for the K of the list that equals v; false (f not called) if none does.
template <int... Ks, class F>
inline bool with_int(int v, F&& f) {
  return ((v == Ks ? (f(std::integral_constant<int, Ks>{}), true) : false) || ...);
}
template <int K> using int_c = std::integral_constant<int, K>;

}  // namespace admm

// "(n,m) " of an X(n, m) shape list: LIST(ADMM_DIM_NAME) is the list's string
#define ADMM_DIM_STR2(x) #x
#define ADMM_DIM_STR(x) ADMM_DIM_STR2(x)
#define ADMM_DIM_NAME(NX, NU) "(" ADMM_DIM_STR(NX) "," ADMM_DIM_STR(NU) ") "
