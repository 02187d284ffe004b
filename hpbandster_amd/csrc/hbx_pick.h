// hbx_pick.h -- the one ladder from a runtime value to a template argument (plain C++17, host side): the
// scoring files turn a prepared KDE's bucket (dc_pad, du_pad, nsc, kc, kp) and its flags into a kernel
// instance through it, one hbx_pick per template parameter, nested.
#pragma once
#include <type_traits>

// f(std::integral_constant<int, V>) for the V of Vs... that equals v; a v outside the list: a value-initialised
// result (nullptr for a kernel pointer, {} for a struct of them).  Every rung returns the type of the first.
// A combination that is not built: the callable tests it with `if constexpr` and returns null itself.
template <int V0, int... Vs, class F>
constexpr auto hbx_pick(int v, F&& f) -> decltype(f(std::integral_constant<int, V0>{})) {
  decltype(f(std::integral_constant<int, V0>{})) r{};
  (void)((v == V0 ? (r = f(std::integral_constant<int, V0>{}), true) : false) || ... ||
         (v == Vs ? (r = f(std::integral_constant<int, Vs>{}), true) : false));
  return r;
}
#define HBX_PICKED(c) (decltype(c)::value)  // the rung's value, a constant expression inside the callable

namespace hbx_pick_test {
struct Two { int a = 0, b = 0; };
constexpr int k3[3] = {30, 40, 50};
constexpr auto ptr = [](auto c) -> const int* { if constexpr (HBX_PICKED(c) == 5) return nullptr; else return &k3[HBX_PICKED(c) - 3]; };
constexpr auto two = [](auto c) { return Two{HBX_PICKED(c), 2 * HBX_PICKED(c)}; };
static_assert(hbx_pick<3, 4, 5>(3, ptr) == &k3[0] && hbx_pick<3, 4, 5>(4, ptr) == &k3[1], "first, middle");
static_assert(hbx_pick<3, 4, 5>(5, ptr) == nullptr && hbx_pick<5, 3, 4>(4, ptr) == &k3[1], "a gated rung; last");
static_assert(hbx_pick<3, 4, 5>(0, ptr) == nullptr && hbx_pick<3, 4, 5>(6, ptr) == nullptr, "a miss: null");
static_assert(hbx_pick<0, 1>(true, two).b == 2 && hbx_pick<0, 1>(7, two).a == 0, "a struct result; its miss: {}");
static_assert(hbx_pick<7>(7, two).a == 7 && hbx_pick<7>(8, two).b == 0, "a one-rung list");
}  // namespace hbx_pick_test
