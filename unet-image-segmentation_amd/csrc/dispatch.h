// Runtime value -> template argument, at the call site.  Each helper calls the generic lambda f
// with std::integral_constant arguments, so the launch it wraps is written out where it is used:
//     with_view(mode, drop, [&](auto M, auto D) { kernel<M(), D()><<<grid, 256, lds, st>>>(args); });
// A combination that must not be instantiated is pruned with `if constexpr` inside the lambda.
// Host-only; no type erasure, no tables: every call is a chain of compares the compiler inlines.
#pragma once
#include <type_traits>
#include <utility>

#include "../../include/unet_hip.h"

namespace unet {

template <int V>
using Int = std::integral_constant<int, V>;

template <class F>
decltype(auto) with_bool(bool b, F&& f) {
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}

// f(Int<V>) for the first V equal to v; the LAST V is the fall-back when none matches
template <int V0, int... Vs, class F>
decltype(auto) with_int(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) {
        return f(Int<V0>{});
    } else {
        if (v == V0) return f(Int<V0>{});
        return with_int<Vs...>(v, f);
    }
}

// f(Int<B>) for the first bound B >= v (ascending bounds); the last bound takes everything above
template <int B0, int... Bs, class F>
decltype(auto) with_bucket(int v, F&& f) {
    if constexpr (sizeof...(Bs) == 0) {
        return f(Int<B0>{});
    } else {
        if (v <= B0) return f(Int<B0>{});
        return with_bucket<Bs...>(v, f);
    }
}

// f(Int<MODE>, bool_constant<DROP>) over the four view modes; any other mode value goes to CONCAT
template <class F>
decltype(auto) with_view(int mode, bool drop, F&& f) {
    return with_int<UNET_VIEW_PLAIN, UNET_VIEW_BNRELU, UNET_VIEW_POOL_BNRELU, UNET_VIEW_CONCAT>(
        mode, [&](auto m) { return with_bool(drop, [&](auto d) { return f(m, d); }); });
}

}  // namespace unet
