// npd_gru_host.hpp -- host side of the RNN decoders: what each kernel family's file (npd_gru.hip, npd_gru_lstm.hip,
// npd_gru_split.hip, npd_gru_split16.hip, npd_gru_wide.hip) exports to the C ABI in npd_gru_api.hip, and the host
// helpers they share.  No device code here.
#pragma once

#include <type_traits>
#include <vector>

#include "npd_gru_common.hpp"
#include "npd_launch.hpp"

namespace npd {
namespace gru {

// ---------------------------------------------------------------------------------- run-time -> compile-time dispatch
// fn(IC<V>{}...) for the Combo<V...> of the list whose values equal v...; only the listed combinations are
// instantiated.  A further parameter (SPLIT, HDT) is a nested dispatch over its own one-value combos.  Returns fn's
// status (NPD_OK where it returns nothing).
template <int... V> struct Combo {};
template <typename... C> struct Combos {};
template <int... V, typename... Rest, typename Fn, typename... Int>
int dispatch(Combos<Combo<V...>, Rest...>, Fn&& fn, Int... v) {
    if (((v == V) && ...)) {
        if constexpr (std::is_void_v<decltype(fn(IC<V>{}...))>) return fn(IC<V>{}...), NPD_OK;
        else return fn(IC<V>{}...);
    }
    if constexpr (sizeof...(Rest) > 0) return dispatch(Combos<Rest...>{}, fn, v...);
    else return fail(NPD_ENOTSUP, "npd_gru: no kernel for this handle's shape");
}
// (F, layers) of the LDS-resident kernels, of the weight-streaming ones, and of every handle.  Every list here and in
// the family files is in the order its kernels have always been instantiated in: the compiler's register allocation
// for a kernel was seen to change with its position among the instantiations of a file
using NarrowShapes = Combos<Combo<64, 2>, Combo<64, 1>, Combo<32, 2>, Combo<32, 1>>;
using WideShapes = Combos<Combo<512, 2>, Combo<512, 1>, Combo<256, 2>, Combo<256, 1>, Combo<128, 2>, Combo<128, 1>>;
using AllShapes = Combos<Combo<512, 2>, Combo<512, 1>, Combo<256, 2>, Combo<256, 1>, Combo<128, 2>, Combo<128, 1>,
                         Combo<64, 2>, Combo<64, 1>, Combo<32, 2>, Combo<32, 1>>;

using npd::launch_lds;  // npd_launch.hpp: shared with the conv family

// ---------------------------------------------------------------------------------- image builders' shared pieces
// the reference's weight vector (npd_gru_create order): per layer W_ih (gates F x din), W_hh (gates F x F), b_ih, b_hh,
// then Linear(F, 1)'s weight and bias.  mats = the three LDS / streamed matrices [L0 hh, L1 ih, L1 hh] (NULL at 1 layer)
struct Weights {
    const float *wih[2], *whh[2], *bih[2], *bhh[2], *wlin, *mats[3];
    float b_lin;
};
inline Weights unpack_weights(const float* W, int gates, int F, int L, int Din) {
    Weights u{};
    for (int l = 0; l < L; ++l) {
        u.wih[l] = W; W += (size_t)gates * F * (l == 0 ? Din : F);
        u.whh[l] = W; W += (size_t)gates * F * F;
        u.bih[l] = W; W += gates * F;
        u.bhh[l] = W; W += gates * F;
    }
    u.wlin = W;
    u.b_lin = W[F];
    u.mats[0] = u.whh[0]; u.mats[1] = u.wih[1]; u.mats[2] = u.whh[1];
    return u;
}

// the matrices' main k-steps in the 32x32x2 A-operand order (image g, tile t, group s / 4, lane l, element s & 3) and the
// fp32 y projection A operands of TT 32-row tiles: k-step s pairs y[s] (lanes 0-31) with y[s + N/2] (lanes 32-63);
// fr(row) = the gate row's factor
template <typename Fr>
void fill_mats(const Weights& u, int NG, int TT, int F, Fr&& fr, std::vector<float>& img) {
    for (int g = 0; g < NG; ++g)
        for (int t = 0; t < TT; ++t)
            for (int s = 0; s < F / 2; ++s)
                for (int l = 0; l < 64; ++l) {
                    const int row = 32 * t + (l & 31);
                    img[((size_t)(g * TT + t) * (F / 8) + s / 4) * 256 + l * 4 + (s & 3)] =
                        fr(row) * u.mats[g][(size_t)row * F + hid_of(s, l >> 5)];
                }
}
template <typename Fr>
void fill_wy(const float* wih0, int TT, int N, int Din, Fr&& fr, std::vector<float>& wy) {
    const int ng = N / 8;
    wy.assign((size_t)TT * ng * 256, 0.0f);
    for (int t = 0; t < TT; ++t)
        for (int s = 0; s < N / 2; ++s)
            for (int l = 0; l < 64; ++l) {
                const int row = 32 * t + (l & 31);
                const int k = s + (l >> 5) * (N / 2);
                wy[((size_t)t * ng + s / 4) * 256 + l * 4 + (s & 3)] = fr(row) * wih0[(size_t)row * Din + k];
            }
}

inline void info_mask(const uint8_t* is_info, int N, uint32_t (&info)[kMaxWords]) {
    for (int w = 0; w < kMaxWords; ++w) info[w] = 0;
    for (int i = 0; i < N; ++i)
        if (is_info[i]) info[i >> 5] |= 1u << (i & 31);
}

// host images of a handle before their upload (img16 / wy16: the 16-codeword split kernel's, or empty)
struct HostImages {
    std::vector<float> img, wy, img16, wy16;
};

// ---------------------------------------------------------------------------------- what the family files export
// Builders that take a handle read its shape and precision and set its image-dependent fields.
// npd_gru.hip: fp32, F <= 64 (build_image serves the split builders and the wide kernels too: every shape)
void build_image(int F, int L, const float* W, int N, int onehot, bool fold, std::vector<float>& img,
                 std::vector<float>& wy, float& b_lin);
void build_head_image(const float* hw, int F, int H, int depth, int hdt, std::vector<float>& img, float& bout);
int launch_f32(const npd_gru* g, const Args& a, hipStream_t s);
// npd_gru_lstm.hip: the image is lstm_wide_kernel's too (every shape); the launch is NarrowShapes without (64, 2)
void build_image_lstm(int F, int L, const float* W, int N, int onehot, std::vector<float>& img, std::vector<float>& wy,
                      float& b_lin);
int launch_lstm(const npd_gru* g, const Args& a, hipStream_t s);
// npd_gru_split.hip (32-codeword waves) and npd_gru_split16.hip (16-codeword waves; F = 64, 2 layers, N % 32 == 0:
// build_image_split16 leaves im.img16 / wy16 empty for other shapes)
void build_image_split(npd_gru& g, const float* W, HostImages& im);
void build_image_split16(npd_gru& g, const float* W, HostImages& im);
int launch_split(const npd_gru* g, const Args& a, hipStream_t s);
// sweep / count mode of the 16-codeword kernel (a.y, a.decoded: n_seg segments; slot: message slot per position, cmp: the
// mask of the compared positions, laid out as Args::info)
int launch_split16_sweep(const npd_gru* g, const Args& a, int n_seg, const float* msg, int K,
                         const uint8_t (&slot)[kMaxN], const uint32_t (&cmp)[kMaxWords], unsigned long long* counters,
                         hipStream_t s);
// npd_gru_wide.hip: F >= 128, and the LSTM at F = 64 x 2
int wide_lds_bytes(int N, int F, int L);
int launch_wide(const npd_gru* g, const Args& a, hipStream_t s);
int launch_lstm_wide(const npd_gru* g, const Args& a, hipStream_t s);

}  // namespace gru
}  // namespace npd
