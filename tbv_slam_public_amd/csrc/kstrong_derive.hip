// kstrong_derive.hip -- the row keys of several k-strongest parameter sets from ONE sweep of the image.
//
// FilterKstrongest (radar_filters.cpp:209-237) keeps the k largest (intensity, range) pairs among the bins >= uchar(z_min) of
// an azimuth; getPeaksFilteredPointCloud (:309-337) drops the kept bins up to ceil(min_distance / range_res) only when it
// builds the cloud.  The bins >= a higher threshold are an upper set of that order, so for k_c <= k_sup and u_c >= u_sup the
// selection of (k_c, u_c) is the top k_c entries of the selection of (k_sup, u_sup), restricted to intensity >= u_c.  A
// parameter grid over (k, z_min, min_distance, range_res) therefore needs one sweep per image -- at (max k, min u), leaving
// the sel_* lists of cfear_kstrong_out -- and this kernel per class: a wavefront per (class, row), lane j holding entry j of
// the row's ascending list, one ballot to rank the kept lanes.  The output is the layout surface_prep_kernel reads from the
// fused sweep (cfear_filter_kstrongest_rowkeys), at a row stride of 64 keys.
#include "common.hpp"
#include "polar_common.hpp"

namespace {

constexpr int kDeriveWaves = 4;            // (class, row) pairs per workgroup

__global__ __launch_bounds__(64 * kDeriveWaves) void kstrong_derive_kernel(const int32_t* __restrict__ sel_range,
                                                                          const uint8_t* __restrict__ sel_intensity,
                                                                          const int32_t* __restrict__ sel_count, const int rows,
                                                                          const int k_sup, const KstrongDeriveClass* __restrict__ classes,
                                                                          const int n_pairs, uint32_t* __restrict__ row_keys,
                                                                          int32_t* __restrict__ row_counts) {
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * kDeriveWaves + (threadIdx.x >> 6);       // wave-uniform
  if (pair >= n_pairs) return;
  const int c = pair / rows, r = pair - c * rows;
  const KstrongDeriveClass cl = classes[c];
  const long long src = (long long)cl.image * rows + r;
  const int count = min(max(sel_count[src], 0), k_sup);                  // k_sup <= 64: one entry per lane
  const bool have = lane < count;
  const int bin = have ? sel_range[src * k_sup + lane] : 0;
  const uint32_t inten = have ? sel_intensity[src * k_sup + lane] : 0u;
  const bool keep = have && lane >= count - cl.k && inten >= (uint32_t)cl.u_zmin && bin > cl.min_range_bin;
  const unsigned long long bal = __ballot(keep);
  if (keep) row_keys[(long long)pair * 64 + __popcll(bal & ((1ull << lane) - 1ull))] = inten << 24 | (uint32_t)bin;
  if (lane == 0) {
    row_counts[(long long)pair * 2] = __popcll(bal);
    row_counts[(long long)pair * 2 + 1] = 0;
  }
}

}  // namespace

int cfear_kstrong_derive_class(const cfear_rowkeys_class* in, int n_images, int k_sup, int u_sup, KstrongDeriveClass* out) {
  if (in->image < 0 || in->image >= n_images || in->k_strongest < 1 || in->k_strongest > k_sup || !(in->range_res > 0.f)) return 0;
  const int u = (int)(uint8_t)(int)in->z_min;                            // radar_driver.cpp:58, radar_filters.cpp:212
  if (u < u_sup) return 0;
  out->image = in->image; out->k = in->k_strongest; out->u_zmin = u;
  out->min_range_bin = (int)std::ceil((double)in->min_distance / (double)in->range_res);   // radar_filters.cpp:315
  return 1;
}

int cfear_kstrong_derive_device(cfear_ctx* ctx, const int32_t* d_sel_range, const uint8_t* d_sel_intensity, const int32_t* d_sel_count,
                                int rows, int k_sup, const KstrongDeriveClass* d_classes, int n_classes, uint32_t* d_row_keys,
                                int32_t* d_row_counts) {
  const long long n_pairs = (long long)n_classes * rows;
  if (n_pairs <= 0) return CFEAR_OK;
  if (n_pairs > 0x7fffffffll - kDeriveWaves) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "row-key derivation: %lld (class, row) pairs", n_pairs);
  ProfScope ps(ctx, "kstrong_derive");
  hipLaunchKernelGGL(kstrong_derive_kernel, dim3((unsigned)((n_pairs + kDeriveWaves - 1) / kDeriveWaves)), dim3(64 * kDeriveWaves), 0,
                     ctx->stream, d_sel_range, d_sel_intensity, d_sel_count, rows, k_sup, d_classes, (int)n_pairs, d_row_keys, d_row_counts);
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

extern "C" int cfear_kstrong_rowkeys_derive(cfear_ctx* ctx, const int32_t* sel_range, const uint8_t* sel_intensity,
                                            const int32_t* sel_count, int32_t n_images, int32_t rows, int32_t k_sup, float z_min_sup,
                                            const cfear_rowkeys_class* classes, int32_t n_classes, uint32_t* row_keys,
                                            int32_t* row_counts) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!sel_range || !sel_intensity || !sel_count || !classes || !row_keys || !row_counts)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (n_images < 1 || rows < 1 || n_classes < 1) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "n_images, rows and n_classes must be >= 1");
  if (k_sup < 1 || k_sup > 64) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "k_sup must be in [1,64]");
  if (cfear_is_device_ptr(classes)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "classes must be host memory");
  if (!cfear_is_device_ptr(sel_range) || !cfear_is_device_ptr(sel_intensity) || !cfear_is_device_ptr(sel_count) ||
      !cfear_is_device_ptr(row_keys) || !cfear_is_device_ptr(row_counts))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "selection lists and outputs must be device memory");
  const int u_sup = (int)(uint8_t)(int)z_min_sup;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsFilter);
  KstrongDeriveClass* d_classes = nullptr;
  st.piece(d_classes, (size_t)n_classes * sizeof(KstrongDeriveClass));
  KstrongDeriveClass* h = (KstrongDeriveClass*)st.record((size_t)n_classes * sizeof(KstrongDeriveClass));
  for (int c = 0; c < n_classes; c++)
    if (!cfear_kstrong_derive_class(&classes[c], n_images, k_sup, u_sup, &h[c]))
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "class %d: image %d of %d, k %d of %d, z_min %g below the sweep's %g, or range_res %g",
                             c, classes[c].image, n_images, classes[c].k_strongest, k_sup, (double)classes[c].z_min, (double)z_min_sup,
                             (double)classes[c].range_res);
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(st.upload(d_classes, h, (size_t)n_classes * sizeof(KstrongDeriveClass)));
  CFEAR_CHECK(cfear_kstrong_derive_device(ctx, sel_range, sel_intensity, sel_count, rows, k_sup, d_classes, n_classes, row_keys, row_counts));
  return st.finish();
}
