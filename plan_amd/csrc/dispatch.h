// Run-time value -> compile-time constant, for choosing a kernel's template instance with the launch written once:
//   ph::dispatch_int<4, 8>(kw, [&](auto KW) { ph::dispatch_bool(sel != nullptr, [&](auto SEL) {
//       kernel<KW(), SEL()><<<grid, 256, 0, stream>>>(...);
//   }); });
// The lists name exactly the instances that exist. No HIP in here: a plain host compiler can include it (tests/test_dispatch.py).
#pragma once

#include <type_traits>

namespace ph {

template <class F>
decltype(auto) dispatch_bool(bool v, F &&f) {
    if (v) return f(std::true_type{});
    return f(std::false_type{});
}

// f(std::integral_constant<int, Vi>{}) for the Vi equal to v; a v that is not listed takes the LAST of the list (a ladder's final else)
template <int V0, int... Vs, class F>
decltype(auto) dispatch_int(int v, F &&f) {
    if constexpr (sizeof...(Vs) == 0) {
        return f(std::integral_constant<int, V0>{});
    } else {
        if (v == V0) return f(std::integral_constant<int, V0>{});
        return dispatch_int<Vs...>(v, f);
    }
}

}  // namespace ph
