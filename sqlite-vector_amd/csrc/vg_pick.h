// vg_pick.h - the kernel tables of the scan variants: (element type, accumulation kind, chunks per lane[, queries per pass]) -> kernel.
//
// One ladder for the single-query kernels (vg_scan.h) and one for the multi-query kernel (vg_scan_multi.h); WHICH kernel template
// a ladder walks is its family - a struct with templated static getters (a function template cannot be a template argument):
//     single-query   template <int VT, int ACC, int U> static scan_fn_t fn();         the register-resident kernel
//                    static const bool has_bits;                                       the table holds the uint8 bit-vector instances (Hamming, Jaccard)
//                    static const bool has_long;                                       rows no shape covers are served ...
//                    template <int VT, int ACC> static scan_fn_t long_fn();            ... by this kernel (only when has_long)
//     multi-query    template <int VT, int ACC, int U, int NQ> static scan_fn_t fn();
// Each kernel has ONE family for all its forms: ScanFamily<FORM, NT, HAS_LONG> (FORM: the VG_SQ_* flags of vg_scan.h, NT: the load
// policy) and MultiFamily<FORM> (FORM: the VG_MQ_* flags of vg_scan_multi.h) below.
// A getter is instantiated only for the combinations a ladder names, and a kernel only where its getter is: the translation unit
// that walks a ladder over a family holds that family's kernels, and exactly these -
//     single-query   all five element types x L2 / cosine / dot / L1 x U in {1, 2, 3, 4, 6, 8}; A_COSN (cached row norms) for
//                    f16 / bf16 only; the long-row kernel without A_COSN; A_HAM / A_JAC (Hamming, Jaccard distance) for uint8 only, long rows included, not in the EX table
//     multi-query    f32 / uint8 / int8 x L2 / cosine / dot / L1, A_HAM / A_JAC for uint8 only; U in {1, 2, 3} at 4 queries per pass, U in {4, 6} at 2
// A combination outside the table is nullptr.
#pragma once

#include "vg_internal.h"

#include "vg_device.h"
#include "vg_scan_multi.h"

template <int FORM, bool NT, bool HAS_LONG>
struct ScanFamily {
    static const bool has_long = HAS_LONG;
    static const bool has_bits = !(FORM & VG_SQ_EX);     // tie_order = reference refuses Hamming and Jaccard before any launch: no EX instances
    template <int VT, int ACC, int U> static scan_fn_t fn() { return vg_scan_kernel<VT, ACC, U, NT, FORM>; }
    template <int VT, int ACC> static scan_fn_t long_fn() { return vg_scan_long_kernel<VT, ACC, NT, FORM>; }
};

template <int FORM>
struct MultiFamily {
    template <int VT, int ACC, int U, int NQ> static scan_fn_t fn() { return vg_scan_multi_kernel<VT, ACC, U, NQ, FORM>; }
};

template <class F, int VT, int ACC>
static scan_fn_t vg_pick_u(int U) {
    switch (U) {
        case 1: return F::template fn<VT, ACC, 1>();
        case 2: return F::template fn<VT, ACC, 2>();
        case 3: return F::template fn<VT, ACC, 3>();
        case 4: return F::template fn<VT, ACC, 4>();
        case 6: return F::template fn<VT, ACC, 6>();
        case 8: return F::template fn<VT, ACC, 8>();
    }
    return nullptr;
}

template <class F, int VT>
static scan_fn_t vg_pick_acc(int acc, int U, bool long_rows) {
    if (long_rows) {
        if constexpr (F::has_long) {
            switch (acc) {
                case A_L2: return F::template long_fn<VT, A_L2>();
                case A_COS: return F::template long_fn<VT, A_COS>();
                case A_DOT: return F::template long_fn<VT, A_DOT>();
                case A_L1: return F::template long_fn<VT, A_L1>();
                case A_HAM:
                    if constexpr (VT == T_U8 && F::has_bits) return F::template long_fn<VT, A_HAM>();
                    return nullptr;
                case A_JAC:
                    if constexpr (VT == T_U8 && F::has_bits) return F::template long_fn<VT, A_JAC>();
                    return nullptr;
            }
        }
        return nullptr;
    }
    switch (acc) {
        case A_L2: return vg_pick_u<F, VT, A_L2>(U);
        case A_COS: return vg_pick_u<F, VT, A_COS>(U);
        case A_DOT: return vg_pick_u<F, VT, A_DOT>(U);
        case A_L1: return vg_pick_u<F, VT, A_L1>(U);
        case A_COSN:
            if constexpr (VT == T_F16 || VT == T_BF16) return vg_pick_u<F, VT, A_COSN>(U);
            return nullptr;
        case A_HAM:
            if constexpr (VT == T_U8 && F::has_bits) return vg_pick_u<F, VT, A_HAM>(U);
            return nullptr;
        case A_JAC:
            if constexpr (VT == T_U8 && F::has_bits) return vg_pick_u<F, VT, A_JAC>(U);
            return nullptr;
    }
    return nullptr;
}

// the single-query kernel of family F for a launch shape
template <class F>
static scan_fn_t vg_pick_scan(int vtype, int acc, int U, bool long_rows) {
    switch (vtype) {
        case VG_TYPE_F32: return vg_pick_acc<F, T_F32>(acc, U, long_rows);
        case VG_TYPE_U8: return vg_pick_acc<F, T_U8>(acc, U, long_rows);
        case VG_TYPE_I8: return vg_pick_acc<F, T_I8>(acc, U, long_rows);
        case VG_TYPE_F16: return vg_pick_acc<F, T_F16>(acc, U, long_rows);
        case VG_TYPE_BF16: return vg_pick_acc<F, T_BF16>(acc, U, long_rows);
    }
    return nullptr;
}

template <class F, int VT, int ACC, int NQ>
static scan_fn_t vg_pick_multi_u(int U) {
    if constexpr (NQ == 4) {
        switch (U) {
            case 1: return F::template fn<VT, ACC, 1, 4>();
            case 2: return F::template fn<VT, ACC, 2, 4>();
            case 3: return F::template fn<VT, ACC, 3, 4>();
        }
    } else {
        switch (U) {
            case 4: return F::template fn<VT, ACC, 4, 2>();
            case 6: return F::template fn<VT, ACC, 6, 2>();
        }
    }
    return nullptr;
}

template <class F, int VT, int NQ>
static scan_fn_t vg_pick_multi_acc(int acc, int U) {
    switch (acc) {
        case A_L2: return vg_pick_multi_u<F, VT, A_L2, NQ>(U);
        case A_COS: return vg_pick_multi_u<F, VT, A_COS, NQ>(U);
        case A_DOT: return vg_pick_multi_u<F, VT, A_DOT, NQ>(U);
        case A_L1: return vg_pick_multi_u<F, VT, A_L1, NQ>(U);
        case A_HAM:
            if constexpr (VT == T_U8) return vg_pick_multi_u<F, VT, A_HAM, NQ>(U);
            return nullptr;
        case A_JAC:
            if constexpr (VT == T_U8) return vg_pick_multi_u<F, VT, A_JAC, NQ>(U);
            return nullptr;
    }
    return nullptr;
}

// the multi-query kernel of family F for NQ (4 or 2) queries per pass
template <class F>
static scan_fn_t vg_pick_multi(int vtype, int acc, int U, int NQ) {
    switch (vtype) {
        case VG_TYPE_F32: return NQ == 4 ? vg_pick_multi_acc<F, T_F32, 4>(acc, U) : vg_pick_multi_acc<F, T_F32, 2>(acc, U);
        case VG_TYPE_U8: return NQ == 4 ? vg_pick_multi_acc<F, T_U8, 4>(acc, U) : vg_pick_multi_acc<F, T_U8, 2>(acc, U);
        case VG_TYPE_I8: return NQ == 4 ? vg_pick_multi_acc<F, T_I8, 4>(acc, U) : vg_pick_multi_acc<F, T_I8, 2>(acc, U);
    }
    return nullptr;
}
