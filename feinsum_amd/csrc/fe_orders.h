// fe_orders.h -- the host-side front end the tetrahedral grad, div and face-mass entry points share (feinsum_hip.hip):
// the table of orders with their launch geometries, the fan over a compile-time field count, the walk over groups of fields
// and the face-mass layout decode.  Host code only; everything resolves at compile time to a switch and direct calls.
#pragma once

#include <cstdint>
#include <type_traits>
#include <utility>

namespace fe {

// One tetrahedral order: Np volume nodes, Nfp nodes per face, and the 16-element sub-tiles per wave tile of the grad, div and
// face-mass kernels (a wave tile is 16 M elements).
template <int NP_, int NFP_, int MG_, int MD_, int MF_>
struct TetOrder {
    static constexpr int NP = NP_, NFP = NFP_, MG = MG_, MD = MD_, MF = MF_;
};
using TetP4 = TetOrder<35, 15, 1, 1, 1>;
using TetP3 = TetOrder<20, 10, 2, 1, 1>;
using TetP2 = TetOrder<10, 6, 3, 3, 2>;
using TetP1 = TetOrder<4, 3, 5, 5, 4>;

constexpr bool is_tet_order(int Np) { return Np == 35 || Np == 20 || Np == 10 || Np == 4; }

// f(row) for the row of Np; the caller has checked is_tet_order(Np).  f is a generic callable: every site that launches a
// kernel over an order's geometry takes NP, NFP and its M from the row, so a geometry cannot differ between two forms.
template <typename F>
auto with_tet_order(int Np, F&& f) {
    switch (Np) {
        case 35: return f(TetP4{});
        case 20: return f(TetP3{});
        case 10: return f(TetP2{});
        default: return f(TetP1{});
    }
}

inline bool is_tet_order(int Np, int Nfp) {
    return is_tet_order(Np) && with_tet_order(Np, [&](auto o) { return Nfp == decltype(o)::NFP; });
}

// f(std::integral_constant<int, nb>) for LO <= nb <= HI, its result in *rc; false (f not called) for any other nb.
template <int LO, int HI, typename F>
bool with_field_count(int nb, int* rc, F&& f) {
    if constexpr (LO > HI) {
        return false;
    } else {
        if (nb == LO) {
            *rc = f(std::integral_constant<int, LO>{});
            return true;
        }
        return with_field_count<LO + 1, HI>(nb, rc, std::forward<F>(f));
    }
}

// The fields 0 .. b-1 of a call in launch groups of up to max_group: f(k0, nb) for each group, in order, until one returns
// non-zero (which is returned).  no_single: never leave a group of one at the end (9 fields in groups of 4: 4 + 3 + 2).
template <typename F>
int for_each_field_group(int b, int max_group, bool no_single, F&& f) {
    for (int k0 = 0; k0 < b;) {
        int nb = b - k0 < max_group ? b - k0 : max_group;
        if (no_single && b - k0 - nb == 1) nb -= 1;
        if (int rc = f(k0, nb)) return rc;
        k0 += nb;
    }
    return 0;
}

// The face-mass layouts of a call (FE_FM_* bits of layout_flags): J[E][nf] or J[nf][ldJ]; the operator as 0 R[f][i][j],
// 1 L[i][f][j], 2 R[f][j][i], 3 L[j][f][i]; and the strides the one-thread-per-entry kernels index them with.
struct FmLayout {
    int jfe, rifj;
    int64_t jEs, jFs;
    int rF, rI, rJ;
    FmLayout(int layout_flags, int Np, int nf, int Nfp, int64_t ldJ)
        : jfe((layout_flags & 1) ? 1 : 0), rifj(((layout_flags & 2) ? 1 : 0) + ((layout_flags & 4) ? 2 : 0)),
          jEs(jfe ? 1 : nf), jFs(jfe ? ldJ : 1),
          rF(rifj == 0 ? Np * Nfp : rifj == 1 ? Nfp : rifj == 2 ? Nfp * Np : Np),
          rI(rifj == 0 ? Nfp : rifj == 1 ? nf * Nfp : 1),
          rJ(rifj == 0 || rifj == 1 ? 1 : rifj == 2 ? Np : nf * Np) {}
};

}  // namespace fe
