// Host-side selectors that turn a runtime value into a compile-time one for a
// generic lambda, so that a launch table reads as a decision list and a kernel
// is instantiated exactly where it is launched (dft.hip, grad_w.hip).
#pragma once

#include <type_traits>

template <int V> using int_c = std::integral_constant<int, V>;

// Calls f(int_c<V>) for the first candidate V that v fits (v <= V), or that
// v equals when EXACT; false when there is none.
template <bool EXACT, int... Vs, typename F>
bool select_first(long v, F&& f) {
  return (((EXACT ? v == Vs : v <= Vs) ? (f(int_c<Vs>{}), true) : false) || ...);
}
template <int... Vs, typename F>
bool select_le(long v, F&& f) { return select_first<false, Vs...>(v, f); }
template <int... Vs, typename F>
bool select_eq(long v, F&& f) { return select_first<true, Vs...>(v, f); }

// Calls f(std::true_type{}) or f(std::false_type{}).
template <typename F>
void select_bool(bool v, F&& f) {
  if (v) f(std::true_type{}); else f(std::false_type{});
}
