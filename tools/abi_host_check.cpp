// The compiler's reading of include/chronoedit_hip.h and include/chronoedit_hip_diag.h: one line `name code code ...` per entry point, a code
// per parameter type - i int, f float, q long long, z size_t, s const char*, A void**, P any other pointer, ? anything else.
// tools/abi_host_check.py generates abi_names.inc (one X(ce_name) line per declared entry point) and compares the output with
// chronoedit_amd.hiplib.header_signatures().  Only decltype(&ce_name) is used: nothing is linked, no HIP, no GPU.
#include <cstddef>
#include <cstdio>
#include <type_traits>

#include "chronoedit_hip.h"
#include "chronoedit_hip_diag.h"

template <class T> constexpr char code() {
    if (std::is_same<T, int>::value) return 'i';
    if (std::is_same<T, float>::value) return 'f';
    if (std::is_same<T, long long>::value) return 'q';
    if (std::is_same<T, size_t>::value) return 'z';
    if (std::is_same<T, const char*>::value) return 's';
    if (std::is_same<T, void**>::value) return 'A';
    if (std::is_pointer<T>::value) return 'P';
    return '?';
}

template <class F> struct S;  // an entry point that does not return int, or is no function, does not compile
template <class... A> struct S<int (*)(A...)> {
    static void print(const char* name) {
        const char codes[] = {code<A>()..., 0};
        std::printf("%s", name);
        for (const char* c = codes; *c; ++c) std::printf(" %c", *c);
        std::printf("\n");
    }
};

int main() {
#define X(n) S<decltype(&n)>::print(#n);
#include "abi_names.inc"
#undef X
    return 0;
}
