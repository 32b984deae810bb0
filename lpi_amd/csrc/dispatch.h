// Run-time dtype codes, flags and row widths -> compile-time template arguments, for the host entry points and the row-job kernel.  A call site lists the
// combinations it instantiates and writes its launch ONCE, in a generic lambda; any other code returns false and calls nothing:
//     if (!dispatch_types(TypeList<Types<float, float>, Types<f16_t, bf16_t>>{}, [&](auto tx, auto ty) { typedef type_of<decltype(tx)> TX; ... }, x_dtype, y_dtype)) return LPI_EINVAL;
#pragma once
#include <type_traits>
#include "common.h"

template <typename T> struct Tag { typedef T type; };
template <typename G> using type_of = typename G::type;
template <typename... T> struct Types {};      // one combination, matched on Elem<T>::DT in order
template <typename... C> struct TypeList {};   // the permitted combinations

template <typename... T, typename F, typename... DT> __host__ __device__ __forceinline__ bool dispatch_one(Types<T...>, F& f, DT... dt) {
    if (!((dt == Elem<T>::DT) && ...)) return false;
    f(Tag<T>{}...);
    return true;
}
template <typename... C, typename F, typename... DT> __host__ __device__ __forceinline__ bool dispatch_types(TypeList<C...>, F f, DT... dt) {
    return (dispatch_one(C{}, f, dt...) || ...);
}
// is (dt...) a listed combination?  (for the callers that check every problem before the first launch)
template <typename L, typename... DT> inline bool types_listed(L, DT... dt) { return dispatch_types(L{}, [](auto...) {}, dt...); }

// run-time flags -> compile-time ones: returns f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...); every combination is instantiated
template <typename F> inline auto dispatch_bool(F f) { return f(); }
template <typename F, typename... B> inline auto dispatch_bool(F f, bool b0, B... rest) {
    return b0 ? dispatch_bool([&](auto... r) { return f(std::true_type{}, r...); }, rest...) : dispatch_bool([&](auto... r) { return f(std::false_type{}, r...); }, rest...);
}

// f(integral_constant<NC>) with the smallest listed chunk bound NC (ascending list) that covers d: ceil(d / 256) <= NC; false if none does
template <int... NC, typename F> __host__ __device__ __forceinline__ bool dispatch_nc(int d, F f) {
    const int nc = (d + 255) / 256;
    return ((nc <= NC ? (f(std::integral_constant<int, NC>{}), true) : false) || ...);
}
// the same for two widths, the ordered pairs NC0 >= NC1 only
template <int... NC, typename F> inline bool dispatch_nc_pair(int d0, int d1, F f) {
    bool ok = false;
    dispatch_nc<NC...>(d0, [&](auto n0) {
        dispatch_nc<NC...>(d1, [&](auto n1) {
            if constexpr (decltype(n0)::value >= decltype(n1)::value) { f(n0, n1); ok = true; }
        });
    });
    return ok;
}
