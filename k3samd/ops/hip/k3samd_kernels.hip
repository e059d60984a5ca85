// k3samd_kernels.hip — torch bindings for the CDNA4 smoke/bench kernels.
//
// Device code lives in stream_kernels.h (shared with the standalone in-pod
// binary native/hipsmoke/mi_stream.hip). These kernels are the MI355X
// analog of the reference stack's in-pod GPU payload (K3S-NVidia runs
// `nvidia-smi` in its validation pod, /root/reference/nvidia-smi.yaml:13).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "atom_kernels.h"
#include "cu_test_kernels.h"
#include "gemm_dense_kernels.h"
#include "gemm_kernels.h"
#include "hostlink_kernels.h"
#include "memtest_kernels.h"
#include "mx_gemm_kernels.h"
#include "stream_kernels.h"

namespace {

using k3samd_kern::f4;

#define K3_CHECK(cond, ...) TORCH_CHECK(cond, "k3samd: ", __VA_ARGS__)

void check_stream_args(const torch::Tensor& t) {
  K3_CHECK(t.is_cuda(), "tensor must be on GPU");
  K3_CHECK(t.scalar_type() == torch::kFloat32, "tensor must be float32");
  K3_CHECK(t.is_contiguous(), "tensor must be contiguous");
  K3_CHECK(t.numel() % 4 == 0, "numel must be divisible by 4");
}

// float4 view of a tensor that passed check_stream_args
f4* f4_ptr(const torch::Tensor& t) {
  return reinterpret_cast<f4*>(t.data_ptr<float>());
}

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// Memory-test target: any contiguous GPU tensor, any dtype, whole 16-byte
// cells. Shape checks come before the device check so they can be
// exercised without a GPU; all of them come before any launch.
int64_t check_mem_buf(const torch::Tensor& t) {
  K3_CHECK(t.is_contiguous(), "buffer must be contiguous");
  K3_CHECK(t.nbytes() % 16 == 0, "buffer byte size must be a multiple of 16");
  K3_CHECK(aligned16(t), "buffer data pointer must be 16-byte aligned");
  K3_CHECK(t.is_cuda(), "buffer must be on GPU");
  return (int64_t)(t.nbytes() / 16);
}

k3samd_kern::MemSpec make_mem_spec(int64_t pattern, uint64_t seed,
                                   bool invert) {
  K3_CHECK(pattern >= 0 && pattern < k3samd_kern::kMemPatternCount,
           "unknown memtest pattern id (0 = ADDR, 1 = WALK, 2 = CHECKER)");
  return k3samd_kern::MemSpec{seed, (int)pattern, invert ? 1 : 0};
}

// The report every test accumulates into; each op adds its device check.
void check_report_shape(const torch::Tensor& report) {
  K3_CHECK(report.scalar_type() == torch::kInt64, "report must be int64");
  K3_CHECK(report.dim() == 1 &&
               report.numel() == k3samd_kern::kMemReportLen &&
               report.is_contiguous(),
           "report must be a contiguous int64[56] from mem_report_new()");
}

void check_mem_report(const torch::Tensor& report, const torch::Tensor& buf) {
  check_report_shape(report);
  K3_CHECK(report.is_cuda() && report.device() == buf.device(),
           "report must be on the same GPU as the buffer");
}

// Verified-GEMM operands: A [M,K] and Bt [N,K], bf16, contiguous, 16-byte
// aligned, meeting gemm_bf16_nt_kernel's shape contract. Everything that
// does not need the device is checked before the device check.
struct GemmDims {
  int64_t m, n, k;
};

GemmDims check_gemm_operands(const torch::Tensor& A, const torch::Tensor& Bt) {
  K3_CHECK(A.scalar_type() == torch::kBFloat16 &&
               Bt.scalar_type() == torch::kBFloat16,
           "A and Bt must be bfloat16");
  K3_CHECK(A.dim() == 2 && Bt.dim() == 2, "A must be [M,K] and Bt [N,K]");
  K3_CHECK(A.is_contiguous() && Bt.is_contiguous(),
           "A and Bt must be contiguous");
  K3_CHECK(A.size(1) == Bt.size(1), "A [M,K] and Bt [N,K] disagree on K");
  GemmDims d{A.size(0), Bt.size(0), A.size(1)};
  K3_CHECK(k3samd_kern::gemm_shape_ok(d.m, d.n, d.k),
           "gemm shape contract: M % 128 == 0, N % 128 == 0, K % 64 == 0, "
           "all > 0");
  K3_CHECK(aligned16(A) && aligned16(Bt),
           "A and Bt data pointers must be 16-byte aligned");
  K3_CHECK(A.is_cuda() && Bt.is_cuda(), "A and Bt must be on GPU");
  K3_CHECK(A.device() == Bt.device(), "A and Bt must be on the same GPU");
  return d;
}

// [M,N] result buffer (fp32 unless a dense format says otherwise): the
// caller's `out` after checks, or a new one.
torch::Tensor gemm_result(const c10::optional<torch::Tensor>& out,
                          const torch::Tensor& A, const GemmDims& d,
                          torch::ScalarType type = torch::kFloat32) {
  if (!out.has_value()) return torch::empty({d.m, d.n}, A.options().dtype(type));
  const torch::Tensor& o = *out;
  K3_CHECK(o.scalar_type() == type, "out must be ",
           type == torch::kInt32     ? "int32"
           : type == torch::kFloat64 ? "float64"
                                     : "float32");
  K3_CHECK(o.dim() == 2 && o.size(0) == d.m && o.size(1) == d.n,
           "out must be [M,N]");
  K3_CHECK(o.is_contiguous(), "out must be contiguous");
  K3_CHECK(aligned16(o), "out data pointer must be 16-byte aligned");
  K3_CHECK(o.is_cuda() && o.device() == A.device(),
           "out must be on the same GPU as A");
  return o;
}

// The optional per-tile placement record of gemm_bf16_nt and mx_gemm_nt:
// int32 [tiles,2] on A's GPU. Returns its data pointer, or null when absent.
void* check_tile_where(const c10::optional<torch::Tensor>& where,
                       const GemmDims& d, const torch::Tensor& A) {
  if (!where.has_value()) return nullptr;
  const torch::Tensor& w = *where;
  const int64_t tiles = (d.m / k3samd_kern::kGemmBM) *
                        (d.n / k3samd_kern::kGemmBN);
  K3_CHECK(w.scalar_type() == torch::kInt32, "where must be int32");
  K3_CHECK(w.dim() == 2 && w.size(0) == tiles && w.size(1) == 2 &&
               w.is_contiguous(),
           "where must be a contiguous int32[tiles,2]");
  K3_CHECK(w.is_cuda() && w.device() == A.device(),
           "where must be on the same GPU as A");
  return w.data_ptr();
}

// The dense format (gemm_dense_kernels.h) of an operand dtype, 0 for none.
int gemm_dense_fmt_of(const torch::Tensor& t) {
  switch (t.scalar_type()) {
    case torch::kFloat16: return k3samd_kern::kGemmFmtFp16;
    case torch::kInt8: return k3samd_kern::kGemmFmtInt8;
    case torch::kFloat32: return k3samd_kern::kGemmFmtFp32;
    case torch::kFloat64: return k3samd_kern::kGemmFmtFp64;
    default: return 0;
  }
}

torch::ScalarType gemm_dense_result_type(int fmt) {
  return fmt == k3samd_kern::kGemmFmtInt8   ? torch::kInt32
         : fmt == k3samd_kern::kGemmFmtFp64 ? torch::kFloat64
                                            : torch::kFloat32;
}

// check_gemm_operands for the dense formats, in the same order; the format
// comes from A's dtype.
GemmDims check_gemm_dense_operands(const torch::Tensor& A,
                                   const torch::Tensor& Bt, int* fmt) {
  *fmt = gemm_dense_fmt_of(A);
  K3_CHECK(*fmt != 0 && Bt.scalar_type() == A.scalar_type(),
           "A and Bt must both be float16, int8, float32 or float64");
  K3_CHECK(A.dim() == 2 && Bt.dim() == 2, "A must be [M,K] and Bt [N,K]");
  K3_CHECK(A.is_contiguous() && Bt.is_contiguous(),
           "A and Bt must be contiguous");
  K3_CHECK(A.size(1) == Bt.size(1), "A [M,K] and Bt [N,K] disagree on K");
  GemmDims d{A.size(0), Bt.size(0), A.size(1)};
  K3_CHECK(k3samd_kern::gemm_dense_shape_ok(*fmt, d.m, d.n, d.k),
           "gemm shape contract: M % 128 == 0, N % 128 == 0, K % ",
           k3samd_kern::gemm_dense_step_k(*fmt), " == 0 (",
           k3samd_kern::gemm_dense_fmt_name(*fmt), "), all > 0");
  K3_CHECK(aligned16(A) && aligned16(Bt),
           "A and Bt data pointers must be 16-byte aligned");
  K3_CHECK(A.is_cuda() && Bt.is_cuda(), "A and Bt must be on GPU");
  K3_CHECK(A.device() == Bt.device(), "A and Bt must be on the same GPU");
  return d;
}

bool is_u8_matrix(const torch::Tensor& t) {
  return t.scalar_type() == torch::kUInt8 && t.dim() == 2;
}

// Verified-MX-GEMM operands: packed elements A [M, KB] and Bt [N, KB]
// (KB = K bytes for fp8, K / 2 for fp4) with E8M0 scales SA [M, K/32] and
// SB [N, K/32], all uint8, contiguous, A and Bt 16-byte aligned, meeting
// mx_gemm_nt_kernel's shape contract. Device checks come last.
GemmDims check_mx_operands(const torch::Tensor& A, const torch::Tensor& SA,
                           const torch::Tensor& Bt, const torch::Tensor& SB,
                           int64_t fmt) {
  K3_CHECK(k3samd_kern::mx_fmt_ok((int)fmt),
           "fmt must be 0 (fp8 e4m3) or 4 (fp4 e2m1)");
  K3_CHECK(is_u8_matrix(A) && is_u8_matrix(SA) && is_u8_matrix(Bt) &&
               is_u8_matrix(SB),
           "A, SA, Bt and SB must be 2-D uint8");
  K3_CHECK(A.is_contiguous() && SA.is_contiguous() && Bt.is_contiguous() &&
               SB.is_contiguous(),
           "A, SA, Bt and SB must be contiguous");
  K3_CHECK(A.size(1) == Bt.size(1), "A and Bt disagree on K");
  GemmDims d{A.size(0), Bt.size(0), fmt == 4 ? 2 * A.size(1) : A.size(1)};
  K3_CHECK(k3samd_kern::mx_shape_ok((int)fmt, d.m, d.n, d.k),
           "mx gemm shape contract: M % 128 == 0, N % 128 == 0, K % 128 == 0 "
           "(fp8) or K % 256 == 0 (fp4), all > 0");
  K3_CHECK(SA.size(0) == d.m && SA.size(1) == d.k / 32 && SB.size(0) == d.n &&
               SB.size(1) == d.k / 32,
           "scales must be SA [M, K/32] and SB [N, K/32]");
  K3_CHECK(aligned16(A) && aligned16(Bt),
           "A and Bt data pointers must be 16-byte aligned");
  K3_CHECK(A.is_cuda() && SA.is_cuda() && Bt.is_cuda() && SB.is_cuda(),
           "A, SA, Bt and SB must be on GPU");
  K3_CHECK(A.device() == SA.device() && A.device() == Bt.device() &&
               A.device() == SB.device(),
           "A, SA, Bt and SB must be on the same GPU");
  return d;
}

// ---- per-CU self-test arguments (cu_test_kernels.h) ----
// Everything that does not need the device is checked before the device
// checks, and all of it before any launch.

void check_cu_rounds(int64_t rounds) {
  K3_CHECK(rounds >= 1 && rounds <= (1 << 30), "rounds must be >= 1 and <= 2^30");
}

// `where` is int32 [rows, 2] with rows = wgs * per_wg; returns wgs.
int64_t check_cu_where_shape(const torch::Tensor& where, int64_t per_wg) {
  K3_CHECK(where.scalar_type() == torch::kInt32, "where must be int32");
  K3_CHECK(where.dim() == 2 && where.size(1) == 2 && where.is_contiguous() &&
               where.size(0) >= per_wg && where.size(0) % per_wg == 0 &&
               k3samd_kern::cu_grid_ok(where.size(0) / per_wg),
           per_wg == 1
               ? "where must be a contiguous int32[wgs,2], 1 <= wgs <= 2^20"
               : "where must be a contiguous int32[4*wgs,2], 1 <= wgs <= 2^20");
  return where.size(0) / per_wg;
}

// Inject list: CPU int64 [n, cols], n <= 256, column j in [0, limit[j]).
// Returns the row count (0 when absent).
int check_cu_inject(const c10::optional<torch::Tensor>& inject, int64_t cols,
                    const int64_t* limit) {
  if (!inject.has_value()) return 0;
  const torch::Tensor& t = *inject;
  K3_CHECK(t.scalar_type() == torch::kInt64 && !t.is_cuda(),
           "inject must be a CPU int64 tensor");
  K3_CHECK(t.dim() == 2 && t.size(1) == cols && t.is_contiguous() &&
               t.size(0) <= k3samd_kern::kCuMaxInject,
           cols == 4 ? "inject must be a contiguous int64[n,4], n <= 256"
                     : "inject must be a contiguous int64[n,5], n <= 256");
  const int64_t* v = t.data_ptr<int64_t>();
  for (int64_t i = 0; i < t.size(0); ++i)
    for (int64_t j = 0; j < cols; ++j)
      K3_CHECK(v[i * cols + j] >= 0 && v[i * cols + j] < limit[j],
               cols == 4 ? "inject row out of range: (wg < wgs, lds_dword < "
                           "40960, xor_mask < 2^32, phase 0..3)"
                         : "inject row out of range: (wg < wgs, wave < 4, "
                           "lane < 64, k 0..4, xor_mask < 2^32)");
  return (int)t.size(0);
}

// Optional int32 output of exactly [rows, cols], 16-byte aligned.
void check_cu_out_shape(const c10::optional<torch::Tensor>& out, int64_t rows,
                        int64_t cols, const char* msg) {
  if (!out.has_value()) return;
  const torch::Tensor& t = *out;
  K3_CHECK(t.scalar_type() == torch::kInt32 && t.dim() == 2 &&
               t.size(0) == rows && t.size(1) == cols && t.is_contiguous(),
           msg);
  K3_CHECK(aligned16(t), "output data pointer must be 16-byte aligned");
}

void check_cu_devices(const torch::Tensor& report, const torch::Tensor& where,
                      const c10::optional<torch::Tensor>& out) {
  K3_CHECK(where.is_cuda(), "where must be on GPU");
  K3_CHECK(report.is_cuda() && report.device() == where.device(),
           "report must be on the same GPU as where");
  K3_CHECK(!out.has_value() ||
               (out->is_cuda() && out->device() == where.device()),
           "dump / sig_out must be on the same GPU as where");
}

// ---- host-link test arguments (hostlink_kernels.h) ----
// Everything that does not need the HIP runtime is checked first, the
// pinned check comes last, and all of it before any launch.

// A host buffer: contiguous CPU tensor of whole `unit`-byte pieces, at least
// one, 16-byte aligned. Returns the byte size.
int64_t check_link_host_shape(const torch::Tensor& t, int64_t unit,
                              const char* size_msg) {
  K3_CHECK(!t.is_cuda(), "host buffer must be a CPU tensor");
  K3_CHECK(t.is_contiguous(), "host buffer must be contiguous");
  K3_CHECK(t.nbytes() > 0 && t.nbytes() % unit == 0, size_msg);
  K3_CHECK(aligned16(t), "host buffer data pointer must be 16-byte aligned");
  return (int64_t)t.nbytes();
}

constexpr const char* kLinkCellMsg =
    "host buffer byte size must be a non-zero multiple of 16";

void check_link_wgs(int64_t wgs, int64_t least) {
  K3_CHECK(wgs >= least && k3samd_kern::link_wgs_ok(wgs),
           least == 1 ? "wgs must be in 1 .. 4096"
                      : "duplex wgs must be in 2 .. 4096");
}

void check_link_report(const torch::Tensor& report) {
  check_report_shape(report);
  K3_CHECK(report.is_cuda(), "report must be on GPU");
}

// With XNACK off a device access to pageable host memory faults the card,
// so a buffer is accepted only when the runtime reports host memory for its
// first and last byte and a device pointer exists. Returns that pointer.
void* link_device_pointer(const torch::Tensor& t) {
  char* host = static_cast<char*>(t.data_ptr());
  void* dev[2] = {nullptr, nullptr};
  bool ok = true;
  for (int end = 0; end < 2 && ok; ++end) {
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    char* p = host + (end ? (int64_t)t.nbytes() - 1 : 0);
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
      (void)hipGetLastError();  // an unregistered pointer is not an error here
      ok = false;
    } else {
      ok = attr.type == hipMemoryTypeHost && attr.devicePointer != nullptr;
      dev[end] = attr.devicePointer;
    }
  }
  ok = ok && static_cast<char*>(dev[1]) - static_cast<char*>(dev[0]) ==
                 (int64_t)t.nbytes() - 1;
  K3_CHECK(ok,
           "host buffer must be pinned (page-locked, device-visible) host "
           "memory: use tensor.pin_memory() or torch.empty(..., "
           "pin_memory=True)");
  return dev[0];
}

void check_chase_n(int64_t n) {
  K3_CHECK(k3samd_kern::link_chase_n_ok(n),
           "chase n must be a power of two in 2 .. 2^26");
}

void check_chase_hops(int64_t hops) {
  K3_CHECK(hops >= 1 && hops <= k3samd_kern::kLinkChaseMaxHops,
           "chase hops must be in 1 .. 2^22");
}

void check_chase_buf(const torch::Tensor& t, int64_t n) {
  check_link_host_shape(t, 64, "chase buffer byte size must be 64 * n");
  K3_CHECK((int64_t)t.nbytes() == 64 * n,
           "chase buffer byte size must be 64 * n");
}

void check_link_threads(int64_t threads) {
  K3_CHECK(threads >= 0 && threads <= k3samd_kern::kLinkMaxHostThreads,
           "threads must be 0 (automatic) .. 16");
}


// ---- global-atomics test arguments (atom_kernels.h) ----
// Everything that does not need the device is checked before the device
// checks, and all of it before any launch.

void check_atom_op(int64_t op, bool reduce) {
  K3_CHECK(k3samd_kern::atom_op_ok((int)op) && op == (int)op,
           "unknown atomics op id (see ops.ATOM_OPS)");
  K3_CHECK(k3samd_kern::atom_is_chain((int)op) != reduce,
           reduce ? "op must be a reduce op, not swap / cas"
                  : "op must be a chain op: swap, swap64, cas or cas64");
}

// A slot buffer of `op`: contiguous, elements of the op's slot size, within
// atom_shape_ok(op, slots, w). Returns the slot count.
int64_t check_atom_buf(const torch::Tensor& t, int64_t op, int64_t w) {
  K3_CHECK(t.is_contiguous(), "buffer must be contiguous");
  K3_CHECK((int64_t)t.element_size() == k3samd_kern::atom_slot_bytes((int)op),
           "buffer element size must be the op's slot size (4 or 8 bytes)");
  K3_CHECK(k3samd_kern::atom_shape_ok((int)op, t.numel(), w),
           "atomics shape contract: 1 <= slots <= 2^30, 1 <= W <= the op's "
           "cap (240 packed, else 4096)");
  return t.numel();
}

void check_atom_report(const torch::Tensor& report, const torch::Tensor& buf) {
  check_report_shape(report);
  K3_CHECK(buf.is_cuda(), "buffer must be on GPU");
  K3_CHECK(report.is_cuda() && report.device() == buf.device(),
           "report must be on the same GPU as the buffer");
}

// int32 [wgs, 2] placement table on the buffer's GPU; returns wgs.
int64_t check_atom_where(const torch::Tensor& where, int64_t wgs_exact,
                         int64_t wgs_max) {
  K3_CHECK(where.scalar_type() == torch::kInt32, "where must be int32");
  K3_CHECK(where.dim() == 2 && where.size(1) == 2 && where.is_contiguous() &&
               where.size(0) >= 1 && where.size(0) <= wgs_max &&
               (wgs_exact == 0 || where.size(0) == wgs_exact),
           wgs_exact ? "where must be a contiguous int32[ceil(draws/256),2]"
                     : "where must be a contiguous int32[wgs,2], 1 <= wgs <= "
                       "65536");
  return where.size(0);
}

struct AtomTicketDims {
  int64_t counters, draws;
  bool wide;
};

AtomTicketDims check_atom_ticket(const torch::Tensor& counters,
                                 const torch::Tensor& tickets) {
  K3_CHECK((counters.scalar_type() == torch::kInt32 ||
            counters.scalar_type() == torch::kInt64) &&
               tickets.scalar_type() == counters.scalar_type(),
           "counters and tickets must both be int32 or both int64");
  K3_CHECK(counters.dim() == 1 && tickets.dim() == 1 &&
               counters.is_contiguous() && tickets.is_contiguous(),
           "counters and tickets must be contiguous and one-dimensional");
  K3_CHECK(counters.numel() >= 1 &&
               counters.numel() <= k3samd_kern::kAtomMaxCounters &&
               tickets.numel() >= 1 &&
               tickets.numel() <= k3samd_kern::kAtomMaxDraws,
           "1 <= counters <= 2^20 and 1 <= draws <= 2^30");
  return {counters.numel(), tickets.numel(),
          counters.scalar_type() == torch::kInt64};
}

// `other` is the where or perm table of the same call.
void check_atom_ticket_devices(const torch::Tensor& counters,
                               const torch::Tensor& tickets,
                               const torch::Tensor& other, const char* msg) {
  K3_CHECK(counters.is_cuda() && tickets.is_cuda() &&
               counters.device() == tickets.device(),
           "counters and tickets must be on the same GPU");
  K3_CHECK(other.is_cuda() && other.device() == counters.device(), msg);
}

}  // namespace

void stream_triad(torch::Tensor a, torch::Tensor b, torch::Tensor c, double s,
                  bool nontemporal) {
  check_stream_args(a);
  check_stream_args(b);
  check_stream_args(c);
  K3_CHECK(a.numel() == b.numel() && a.numel() == c.numel(), "size mismatch");
  k3samd_kern::launch_stream_triad(at::hip::getCurrentHIPStream(), f4_ptr(a),
                                   f4_ptr(b), f4_ptr(c), (float)s,
                                   a.numel() / 4, nontemporal);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void stream_copy(torch::Tensor a, torch::Tensor b, bool nontemporal) {
  check_stream_args(a);
  check_stream_args(b);
  K3_CHECK(a.numel() == b.numel(), "size mismatch");
  k3samd_kern::launch_stream_copy(at::hip::getCurrentHIPStream(), f4_ptr(a),
                                  f4_ptr(b), a.numel() / 4, nontemporal);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void stream_scale(torch::Tensor a, torch::Tensor c, double s, bool nontemporal) {
  check_stream_args(a);
  check_stream_args(c);
  K3_CHECK(a.numel() == c.numel(), "size mismatch");
  k3samd_kern::launch_stream_scale(at::hip::getCurrentHIPStream(), f4_ptr(a),
                                   f4_ptr(c), (float)s, a.numel() / 4,
                                   nontemporal);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void stream_add(torch::Tensor a, torch::Tensor b, torch::Tensor c,
                bool nontemporal) {
  check_stream_args(a);
  check_stream_args(b);
  check_stream_args(c);
  K3_CHECK(a.numel() == b.numel() && a.numel() == c.numel(), "size mismatch");
  k3samd_kern::launch_stream_add(at::hip::getCurrentHIPStream(), f4_ptr(a),
                                 f4_ptr(b), f4_ptr(c), a.numel() / 4,
                                 nontemporal);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// Launch `out.numel()` blocks x 256 threads, `iters` MFMA quads each.
// Returns total FLOPs issued so the caller can compute TFLOP/s.
double mfma_throughput(torch::Tensor out, int64_t iters, int64_t shape) {
  K3_CHECK(out.is_cuda() && out.scalar_type() == torch::kFloat32 &&
               out.is_contiguous(),
           "out must be contiguous float32 GPU tensor");
  K3_CHECK(shape == 16 || shape == 32 || shape == 8 || shape == 4,
           "shape must be 16, 32 (bf16), 8 (MX-fp8) or 4 (MX-fp4)");
  int64_t blocks = out.numel();
  K3_CHECK(blocks > 0 && blocks <= (1 << 22), "bad block count");
  const auto kind = static_cast<k3samd_kern::MfmaKind>(shape);
  k3samd_kern::launch_mfma_throughput(at::hip::getCurrentHIPStream(), kind,
                                      out.data_ptr<float>(), (int)blocks,
                                      (int)iters);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return k3samd_kern::mfma_throughput_flops(kind, blocks, iters);
}

torch::Tensor mfma_gemm16(torch::Tensor A, torch::Tensor B, int64_t layout) {
  K3_CHECK(A.is_cuda() && B.is_cuda(), "A,B must be on GPU");
  K3_CHECK(A.scalar_type() == torch::kBFloat16 &&
               B.scalar_type() == torch::kBFloat16,
           "A,B must be bf16");
  K3_CHECK(A.is_contiguous() && B.is_contiguous(), "A,B must be contiguous");
  K3_CHECK(A.size(0) == 16 && A.size(1) == 32 && B.size(0) == 32 &&
               B.size(1) == 16,
           "A must be [16,32], B [32,16]");
  auto D = torch::empty({16, 16}, A.options().dtype(torch::kFloat32));
  k3samd_kern::launch_mfma_gemm16(at::hip::getCurrentHIPStream(),
                                  A.data_ptr(), B.data_ptr(),
                                  D.data_ptr<float>(), (int)layout);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return D;
}

// Block-scaled MX single-tile GEMM: D[16,16] = A[16,128] x B[128,16]
// with fp8-e4m3 (fmt=0) or fp4-e2m1 (fmt=4) operands, unit scales.
// A: uint8 [16,128] (fp8) / [16,64] (fp4, 2 elems per byte, low nibble =
// even k). B: uint8 packed COLUMN-major with k contiguous: [16,128]
// (fp8: row c holds column c of B) / [16,64] (fp4).
torch::Tensor mx_gemm16(torch::Tensor A, torch::Tensor B, int64_t fmt) {
  K3_CHECK(A.is_cuda() && B.is_cuda(), "A,B must be on GPU");
  K3_CHECK(A.scalar_type() == torch::kUInt8 &&
               B.scalar_type() == torch::kUInt8,
           "A,B must be uint8 (packed fp8/fp4)");
  K3_CHECK(A.is_contiguous() && B.is_contiguous(), "A,B must be contiguous");
  K3_CHECK(fmt == 0 || fmt == 4, "fmt must be 0 (fp8 e4m3) or 4 (fp4)");
  int64_t kb = fmt == 0 ? 128 : 64;  // packed bytes along k
  K3_CHECK(A.size(0) == 16 && A.size(1) == kb && B.size(0) == 16 &&
               B.size(1) == kb,
           "A must be [16,KB], B [16,KB] (B column-major-packed)");
  auto D = torch::empty({16, 16}, A.options().dtype(torch::kFloat32));
  k3samd_kern::launch_mx_gemm16(at::hip::getCurrentHIPStream(), (int)fmt,
                                A.data_ptr(), B.data_ptr(),
                                D.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return D;
}

// ---- HBM pattern memory test (memtest_kernels.h) ----
// None of these synchronise with the host: a multi-pass march queues every
// step on the current stream and reads the report once at the end.

void mem_fill(torch::Tensor buf, int64_t pattern, uint64_t seed, bool invert,
              uint64_t cell_offset, bool nontemporal) {
  auto spec = make_mem_spec(pattern, seed, invert);
  int64_t n_cells = check_mem_buf(buf);
  k3samd_kern::launch_mem_fill(at::hip::getCurrentHIPStream(), buf.data_ptr(),
                               n_cells, cell_offset, spec, nontemporal);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void mem_verify(torch::Tensor buf, torch::Tensor report, int64_t pattern,
                uint64_t seed, bool invert, uint64_t cell_offset) {
  auto spec = make_mem_spec(pattern, seed, invert);
  int64_t n_cells = check_mem_buf(buf);
  check_mem_report(report, buf);
  k3samd_kern::launch_mem_verify(at::hip::getCurrentHIPStream(),
                                 buf.data_ptr(), n_cells, cell_offset, spec,
                                 report.data_ptr());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void mem_verify_fill(torch::Tensor buf, torch::Tensor report,
                     int64_t old_pattern, uint64_t old_seed, bool old_invert,
                     int64_t new_pattern, uint64_t new_seed, bool new_invert,
                     uint64_t cell_offset, bool nontemporal) {
  auto old_spec = make_mem_spec(old_pattern, old_seed, old_invert);
  auto new_spec = make_mem_spec(new_pattern, new_seed, new_invert);
  int64_t n_cells = check_mem_buf(buf);
  check_mem_report(report, buf);
  k3samd_kern::launch_mem_verify_fill(at::hip::getCurrentHIPStream(),
                                      buf.data_ptr(), n_cells, cell_offset,
                                      old_spec, new_spec, report.data_ptr(),
                                      nontemporal);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// ---- verified bf16 MFMA GEMM (gemm_kernels.h) ----
// Like the memtest ops, none of these synchronise with the host.

// `buf` is the stored [rows, cols] bf16 matrix: A[M,K] for which = 0,
// Bt[N,K] for which = 1 (element [n][k] = gemm_operand(seed, 1, k, n)).
void gemm_fill(torch::Tensor buf, int64_t which, uint64_t seed, int64_t rows,
               int64_t cols) {
  K3_CHECK(which == 0 || which == 1, "which must be 0 (A) or 1 (Bt)");
  const int fmt = gemm_dense_fmt_of(buf);  // 0: the bf16 path
  K3_CHECK(fmt != 0 || buf.scalar_type() == torch::kBFloat16,
           "buffer must be bfloat16");
  const int per_cell = fmt ? 16 / k3samd_kern::gemm_dense_elem_bytes(fmt) : 8;
  K3_CHECK(rows > 0 && cols > 0 && cols % per_cell == 0 && rows <= (1 << 24) &&
               cols <= (1 << 24),
           "rows and cols must be > 0 and cols a multiple of ", per_cell);
  K3_CHECK(buf.numel() == rows * cols, "buffer must hold rows * cols elements");
  check_mem_buf(buf);
  if (fmt)
    k3samd_kern::launch_gemm_dense_fill(at::hip::getCurrentHIPStream(), fmt,
                                        buf.data_ptr(), (int)which, seed, rows,
                                        cols);
  else
    k3samd_kern::launch_gemm_fill(at::hip::getCurrentHIPStream(),
                                  buf.data_ptr(), (int)which, seed, rows, cols);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// C[M,N] fp32 = A[M,K] . Bt[N,K]^T on the matrix pipes; any bf16 data.
// `where` (optional int32 [tiles,2], tile = (m/128)*(N/128) + n/128)
// receives the XCC_ID and HW_ID registers of each tile's workgroup.
torch::Tensor gemm_bf16_nt(torch::Tensor A, torch::Tensor Bt,
                           c10::optional<torch::Tensor> out,
                           c10::optional<torch::Tensor> where) {
  GemmDims d = check_gemm_operands(A, Bt);
  void* where_ptr = check_tile_where(where, d, A);
  torch::Tensor C = gemm_result(out, A, d);
  k3samd_kern::launch_gemm_bf16_nt(at::hip::getCurrentHIPStream(),
                                   A.data_ptr(), Bt.data_ptr(), C.data_ptr(),
                                   where_ptr, d.m, d.n, d.k);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return C;
}

// The same product in int32 VALU arithmetic (no MFMA), written as fp32.
// Operands must hold integers in [-128, 127]; K <= 32768 keeps every sum
// of generator operands exactly representable.
torch::Tensor gemm_ref_int(torch::Tensor A, torch::Tensor Bt,
                           c10::optional<torch::Tensor> out) {
  K3_CHECK(A.dim() != 2 || A.size(1) <= k3samd_kern::kGemmExactMaxK,
           "gemm_ref_int needs K <= 32768 (exactness bound 256*K <= 2^23)");
  GemmDims d = check_gemm_operands(A, Bt);
  torch::Tensor gold = gemm_result(out, A, d);
  k3samd_kern::launch_gemm_ref_int(at::hip::getCurrentHIPStream(),
                                   A.data_ptr(), Bt.data_ptr(),
                                   gold.data_ptr(), d.m, d.n, d.k);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return gold;
}

// ---- verified fp16 / int8 / fp32 / fp64 GEMM (gemm_dense_kernels.h) ----
// The format follows A's dtype; C is float32, int32, float32 or float64.

// C[M,N] = A[M,K] . Bt[N,K]^T on the format's matrix pipe; any data.
// `where` as for gemm_bf16_nt.
torch::Tensor gemm_dense_nt(torch::Tensor A, torch::Tensor Bt,
                            c10::optional<torch::Tensor> out,
                            c10::optional<torch::Tensor> where) {
  int fmt;
  GemmDims d = check_gemm_dense_operands(A, Bt, &fmt);
  void* where_ptr = check_tile_where(where, d, A);
  torch::Tensor C = gemm_result(out, A, d, gemm_dense_result_type(fmt));
  k3samd_kern::launch_gemm_dense_nt(at::hip::getCurrentHIPStream(), fmt,
                                    A.data_ptr(), Bt.data_ptr(), C.data_ptr(),
                                    where_ptr, d.m, d.n, d.k);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return C;
}

// The same product in int32 VALU arithmetic (no MFMA). Operands must hold
// integers in [-128, 127]; K <= 32768 keeps every sum within int32, and
// every sum of generator operands exactly representable in fp32.
torch::Tensor gemm_dense_ref_int(torch::Tensor A, torch::Tensor Bt,
                                 c10::optional<torch::Tensor> out) {
  K3_CHECK(A.dim() != 2 || A.size(1) <= k3samd_kern::kGemmExactMaxK,
           "gemm_dense_ref_int needs K <= 32768 (exactness bound 256*K <= "
           "2^23)");
  int fmt;
  GemmDims d = check_gemm_dense_operands(A, Bt, &fmt);
  torch::Tensor gold = gemm_result(out, A, d, gemm_dense_result_type(fmt));
  k3samd_kern::launch_gemm_dense_ref_int(at::hip::getCurrentHIPStream(), fmt,
                                         A.data_ptr(), Bt.data_ptr(),
                                         gold.data_ptr(), d.m, d.n, d.k);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return gold;
}

// Bitwise compare of two equally sized buffers into the memtest report;
// the report's dword index is the index of the 32-bit element.
void buf_compare(torch::Tensor buf, torch::Tensor expected,
                 torch::Tensor report) {
  K3_CHECK(buf.nbytes() == expected.nbytes(),
           "buffer and expected must have the same byte size");
  int64_t n_cells = check_mem_buf(buf);
  check_mem_buf(expected);
  K3_CHECK(expected.device() == buf.device(),
           "expected must be on the same GPU as the buffer");
  check_mem_report(report, buf);
  k3samd_kern::launch_buf_compare(at::hip::getCurrentHIPStream(),
                                  buf.data_ptr(), expected.data_ptr(), n_cells,
                                  report.data_ptr());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// ---- verified MX (fp8 / fp4 block-scaled) MFMA GEMM (mx_gemm_kernels.h) ----
// Like the bf16 ops, none of these synchronise with the host.

// One tile D[16,16] = (A o SA) . (B o SB) with per-lane scale operands.
// A and B packed as for mx_gemm16 ([16,128] fp8 / [16,64] fp4, B
// column-major with k contiguous); SA and SB uint8 [16,4]: the E8M0 scale
// of (row or column, block of 32 k).
torch::Tensor mx_gemm16_scaled(torch::Tensor A, torch::Tensor SA,
                               torch::Tensor B, torch::Tensor SB,
                               int64_t fmt) {
  K3_CHECK(k3samd_kern::mx_fmt_ok((int)fmt),
           "fmt must be 0 (fp8 e4m3) or 4 (fp4 e2m1)");
  K3_CHECK(is_u8_matrix(A) && is_u8_matrix(SA) && is_u8_matrix(B) &&
               is_u8_matrix(SB),
           "A, SA, B and SB must be 2-D uint8");
  K3_CHECK(A.is_contiguous() && SA.is_contiguous() && B.is_contiguous() &&
               SB.is_contiguous(),
           "A, SA, B and SB must be contiguous");
  const int64_t kb = fmt == 0 ? 128 : 64;  // packed bytes along k
  K3_CHECK(A.size(0) == 16 && A.size(1) == kb && B.size(0) == 16 &&
               B.size(1) == kb,
           "A must be [16,KB], B [16,KB] (B column-major-packed)");
  K3_CHECK(SA.size(0) == 16 && SA.size(1) == 4 && SB.size(0) == 16 &&
               SB.size(1) == 4,
           "SA and SB must be [16,4]");
  K3_CHECK(A.is_cuda() && SA.is_cuda() && B.is_cuda() && SB.is_cuda(),
           "A, SA, B and SB must be on GPU");
  K3_CHECK(A.device() == SA.device() && A.device() == B.device() &&
               A.device() == SB.device(),
           "A, SA, B and SB must be on the same GPU");
  auto D = torch::empty({16, 16}, A.options().dtype(torch::kFloat32));
  k3samd_kern::launch_mx_gemm16_scaled(at::hip::getCurrentHIPStream(),
                                       (int)fmt, A.data_ptr(), SA.data_ptr(),
                                       B.data_ptr(), SB.data_ptr(),
                                       D.data_ptr());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return D;
}

// `elems` is the stored [rows, k] element matrix (k bytes per row for fp8,
// k / 2 for fp4) and `scales` its uint8 [rows, k/32]: A and SA for
// which = 0, Bt and SB for which = 1.
void mx_fill(torch::Tensor elems, torch::Tensor scales, int64_t which,
             uint64_t seed, int64_t rows, int64_t k, int64_t fmt) {
  K3_CHECK(k3samd_kern::mx_fmt_ok((int)fmt),
           "fmt must be 0 (fp8 e4m3) or 4 (fp4 e2m1)");
  K3_CHECK(which == 0 || which == 1, "which must be 0 (A) or 1 (Bt)");
  K3_CHECK(elems.scalar_type() == torch::kUInt8 &&
               scales.scalar_type() == torch::kUInt8,
           "elems and scales must be uint8");
  K3_CHECK(rows > 0 && k > 0 && k % 32 == 0 && rows <= (1 << 24) &&
               k <= (1 << 24),
           "rows and k must be > 0 and k a multiple of 32");
  K3_CHECK(elems.numel() == rows * k3samd_kern::mx_row_bytes((int)fmt, k),
           "elems must hold rows * k elements");
  K3_CHECK(scales.numel() == rows * (k / 32),
           "scales must hold rows * k / 32 bytes");
  K3_CHECK(scales.is_contiguous(), "scales must be contiguous");
  check_mem_buf(elems);
  K3_CHECK(scales.is_cuda() && scales.device() == elems.device(),
           "scales must be on the same GPU as elems");
  k3samd_kern::launch_mx_fill(at::hip::getCurrentHIPStream(), elems.data_ptr(),
                              scales.data_ptr(), (int)which, seed, rows, k,
                              (int)fmt);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// C[M,N] fp32 = (A o SA) . (Bt o SB)^T on the matrix pipes; any finite
// element codes and scales. `where` as for gemm_bf16_nt.
torch::Tensor mx_gemm_nt(torch::Tensor A, torch::Tensor SA, torch::Tensor Bt,
                         torch::Tensor SB, int64_t fmt,
                         c10::optional<torch::Tensor> out,
                         c10::optional<torch::Tensor> where) {
  GemmDims d = check_mx_operands(A, SA, Bt, SB, fmt);
  void* where_ptr = check_tile_where(where, d, A);
  torch::Tensor C = gemm_result(out, A, d);
  k3samd_kern::launch_mx_gemm_nt(at::hip::getCurrentHIPStream(), (int)fmt,
                                 A.data_ptr(), SA.data_ptr(), Bt.data_ptr(),
                                 SB.data_ptr(), C.data_ptr(), where_ptr, d.m,
                                 d.n, d.k);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return C;
}

// The same product in int32 VALU arithmetic (no MFMA), written as fp32.
// Elements must decode to integers (fp8) or be any e2m1 code (fp4), scales
// must be 127..129, and K <= 8192 keeps every sum exactly representable.
torch::Tensor mx_gemm_ref_int(torch::Tensor A, torch::Tensor SA,
                              torch::Tensor Bt, torch::Tensor SB, int64_t fmt,
                              c10::optional<torch::Tensor> out) {
  K3_CHECK(A.dim() != 2 || (fmt == 4 ? 2 : 1) * A.size(1) <=
                               k3samd_kern::kMxExactMaxK,
           "mx_gemm_ref_int needs K <= 8192 (exactness bound 1024*K <= 2^23)");
  GemmDims d = check_mx_operands(A, SA, Bt, SB, fmt);
  torch::Tensor gold = gemm_result(out, A, d);
  k3samd_kern::launch_mx_gemm_ref_int(at::hip::getCurrentHIPStream(), (int)fmt,
                                      A.data_ptr(), SA.data_ptr(),
                                      Bt.data_ptr(), SB.data_ptr(),
                                      gold.data_ptr(), d.m, d.n, d.k);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return gold;
}

// ---- per-CU self-test (cu_test_kernels.h) ----
// Like the memtest ops these do not synchronise with the host, apart from
// the copy of a non-empty inject list to the device.

void cu_lds_march(torch::Tensor report, torch::Tensor where, uint64_t seed,
                  int64_t passes, int64_t stop_after,
                  c10::optional<torch::Tensor> inject,
                  c10::optional<torch::Tensor> dump) {
  check_report_shape(report);
  const int64_t wgs = check_cu_where_shape(where, 1);
  K3_CHECK(passes >= 1 && passes <= (1 << 20), "passes must be >= 1 and <= 2^20");
  K3_CHECK(stop_after >= 0 && stop_after <= 4, "stop_after must be 0..4");
  const int64_t limit[4] = {wgs, k3samd_kern::kCuLdsDwords, 1ll << 32, 4};
  const int n_inject = check_cu_inject(inject, 4, limit);
  check_cu_out_shape(dump, wgs, k3samd_kern::kCuLdsDwords,
                     "dump must be a contiguous int32[wgs,40960]");
  check_cu_devices(report, where, dump);
  torch::Tensor inj;
  if (n_inject > 0) inj = inject->to(where.device());
  k3samd_kern::launch_cu_lds_march(
      at::hip::getCurrentHIPStream(), report.data_ptr(), where.data_ptr(), wgs,
      seed, (int)passes, (int)stop_after,
      n_inject > 0 ? inj.data_ptr() : nullptr, n_inject,
      dump.has_value() ? dump->data_ptr() : nullptr);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void cu_valu_signature(torch::Tensor report, torch::Tensor where, uint64_t seed,
                       int64_t rounds, torch::Tensor expected,
                       c10::optional<torch::Tensor> sig_out,
                       c10::optional<torch::Tensor> inject) {
  check_report_shape(report);
  const int64_t wgs = check_cu_where_shape(where, k3samd_kern::kCuWaves);
  check_cu_rounds(rounds);
  K3_CHECK(expected.scalar_type() == torch::kInt32 && expected.dim() == 2 &&
               expected.size(0) == k3samd_kern::kCuWaveLanes &&
               expected.size(1) == 4 && expected.is_contiguous(),
           "expected must be a contiguous int32[64,4] from "
           "cu_signature_expected()");
  K3_CHECK(aligned16(expected),
           "expected data pointer must be 16-byte aligned");
  const int64_t limit[5] = {wgs, k3samd_kern::kCuWaves,
                            k3samd_kern::kCuWaveLanes, 5, 1ll << 32};
  const int n_inject = check_cu_inject(inject, 5, limit);
  check_cu_out_shape(sig_out, wgs * k3samd_kern::kCuWgThreads, 4,
                     "sig_out must be a contiguous int32[256*wgs,4]");
  check_cu_devices(report, where, sig_out);
  K3_CHECK(expected.is_cuda() && expected.device() == where.device(),
           "expected must be on the same GPU as where");
  torch::Tensor inj;
  if (n_inject > 0) inj = inject->to(where.device());
  k3samd_kern::launch_cu_valu_signature(
      at::hip::getCurrentHIPStream(), report.data_ptr(), where.data_ptr(), wgs,
      seed, (int)rounds, expected.data_ptr(),
      sig_out.has_value() ? sig_out->data_ptr() : nullptr,
      n_inject > 0 ? inj.data_ptr() : nullptr, n_inject);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// Host code only (cu_pattern.h): the 64 cells of one wave as a CPU
// int32[64,4] of bit patterns. Needs no GPU.
torch::Tensor cu_signature_expected(uint64_t seed, int64_t rounds) {
  check_cu_rounds(rounds);
  k3samd_kern::CuSigCell cells[k3samd_kern::kCuWaveLanes];
  k3samd_kern::cu_signature_wave(seed, (uint32_t)rounds, cells);
  auto out = torch::empty({k3samd_kern::kCuWaveLanes, 4},
                          torch::dtype(torch::kInt32));
  std::memcpy(out.data_ptr(), cells, sizeof(cells));
  return out;
}

// ---- host-link (PCIe) test (hostlink_kernels.h, hostlink_pattern.h) ----
// The kernels run on the current device and stream and do not synchronise
// with the host; every host buffer is pinned CPU memory.

void link_pull_verify(torch::Tensor host_buf, torch::Tensor report,
                      int64_t pattern, uint64_t seed, bool invert,
                      uint64_t cell_offset, int64_t wgs) {
  auto spec = make_mem_spec(pattern, seed, invert);
  check_link_wgs(wgs, 1);
  const int64_t n_cells = check_link_host_shape(host_buf, 16, kLinkCellMsg) / 16;
  check_link_report(report);
  void* dev = link_device_pointer(host_buf);
  k3samd_kern::launch_link_pull_verify(at::hip::getCurrentHIPStream(), dev,
                                       n_cells, cell_offset, spec,
                                       report.data_ptr(), (int)wgs);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void link_push_fill(torch::Tensor host_buf, int64_t pattern, uint64_t seed,
                    bool invert, uint64_t cell_offset, int64_t wgs) {
  auto spec = make_mem_spec(pattern, seed, invert);
  check_link_wgs(wgs, 1);
  const int64_t n_cells = check_link_host_shape(host_buf, 16, kLinkCellMsg) / 16;
  void* dev = link_device_pointer(host_buf);
  k3samd_kern::launch_link_push_fill(at::hip::getCurrentHIPStream(), dev,
                                     n_cells, cell_offset, spec, (int)wgs);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void link_duplex(torch::Tensor pull_buf, torch::Tensor report,
                 int64_t pull_pattern, uint64_t pull_seed, bool pull_invert,
                 uint64_t pull_cell_offset, torch::Tensor push_buf,
                 int64_t push_pattern, uint64_t push_seed, bool push_invert,
                 uint64_t push_cell_offset, int64_t wgs) {
  auto pull_spec = make_mem_spec(pull_pattern, pull_seed, pull_invert);
  auto push_spec = make_mem_spec(push_pattern, push_seed, push_invert);
  check_link_wgs(wgs, 2);
  const int64_t pull_bytes = check_link_host_shape(pull_buf, 16, kLinkCellMsg);
  const int64_t push_bytes = check_link_host_shape(push_buf, 16, kLinkCellMsg);
  const auto a = reinterpret_cast<uintptr_t>(pull_buf.data_ptr());
  const auto b = reinterpret_cast<uintptr_t>(push_buf.data_ptr());
  K3_CHECK(a + (uintptr_t)pull_bytes <= b || b + (uintptr_t)push_bytes <= a,
           "duplex pull and push regions must not overlap");
  check_link_report(report);
  k3samd_kern::LinkRegion pull{link_device_pointer(pull_buf), pull_bytes / 16,
                               pull_cell_offset, pull_spec};
  k3samd_kern::LinkRegion push{link_device_pointer(push_buf), push_bytes / 16,
                               push_cell_offset, push_spec};
  k3samd_kern::launch_link_duplex(at::hip::getCurrentHIPStream(), pull, push,
                                  report.data_ptr(), (int)wgs);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// `out` is a GPU int64[4]: final index, XOR of visited indices,
// wall_clock64 ticks, hops.
void link_chase(torch::Tensor host_buf, int64_t n, int64_t hops,
                torch::Tensor out) {
  check_chase_n(n);
  check_chase_hops(hops);
  check_chase_buf(host_buf, n);
  K3_CHECK(out.scalar_type() == torch::kInt64 && out.dim() == 1 &&
               out.numel() == k3samd_kern::kLinkChaseOutLen &&
               out.is_contiguous(),
           "out must be a contiguous int64[4]");
  K3_CHECK(out.is_cuda(), "out must be on GPU");
  void* dev = link_device_pointer(host_buf);
  k3samd_kern::launch_link_chase(at::hip::getCurrentHIPStream(), dev,
                                 (uint32_t)n, (uint64_t)hops, out.data_ptr());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// wall_clock64() ticks per millisecond on `device`.
int64_t link_wall_clock_khz(int64_t device) {
  int khz = 0;
  K3_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate,
                                 (int)device) == hipSuccess && khz > 0,
           "the device reports no wall clock rate");
  return khz;
}

// Host code only from here (hostlink_pattern.h): no HIP call, no GPU.

void link_host_fill(torch::Tensor buf, int64_t pattern, uint64_t seed,
                    bool invert, uint64_t cell_offset, int64_t threads) {
  auto spec = make_mem_spec(pattern, seed, invert);
  check_link_threads(threads);
  const int64_t n_cells = check_link_host_shape(buf, 16, kLinkCellMsg) / 16;
  pybind11::gil_scoped_release nogil;
  k3samd_kern::host_fill(buf.data_ptr(), n_cells, spec, cell_offset,
                         (int)threads);
}

// Returns a CPU int64[56] report (the layout mem_report_read() decodes).
torch::Tensor link_host_verify(torch::Tensor buf, int64_t pattern,
                               uint64_t seed, bool invert,
                               uint64_t cell_offset, int64_t threads) {
  auto spec = make_mem_spec(pattern, seed, invert);
  check_link_threads(threads);
  const int64_t n_cells = check_link_host_shape(buf, 16, kLinkCellMsg) / 16;
  auto report = torch::empty({k3samd_kern::kMemReportLen},
                             torch::dtype(torch::kInt64));
  static_assert(sizeof(long long) == sizeof(int64_t), "report element");
  auto* r = reinterpret_cast<long long*>(report.data_ptr<int64_t>());
  k3samd_kern::host_report_reset(r);
  pybind11::gil_scoped_release nogil;
  k3samd_kern::host_verify(buf.data_ptr(), n_cells, spec, cell_offset, r,
                           (int)threads);
  return report;
}

void link_chase_fill(torch::Tensor buf, int64_t n, uint64_t seed) {
  check_chase_n(n);
  check_chase_buf(buf, n);
  k3samd_kern::link_chase_fill(buf.data_ptr(), (uint32_t)n, seed);
}

std::tuple<int64_t, int64_t> link_chase_expected(int64_t n, uint64_t seed,
                                                 int64_t hops) {
  check_chase_n(n);
  check_chase_hops(hops);
  auto r = k3samd_kern::link_chase_expected((uint32_t)n, seed, (uint64_t)hops);
  return {(int64_t)r.final_index, (int64_t)r.xor_all};
}

// ---- global-atomics integrity test (atom_kernels.h, atom_pattern.h) ----
// Like the memtest ops none of these synchronises with the host.

void atom_fill(torch::Tensor buf, int64_t op, uint64_t seed) {
  K3_CHECK(k3samd_kern::atom_op_ok((int)op) && op == (int)op,
           "unknown atomics op id (see ops.ATOM_OPS)");
  const int64_t slots = check_atom_buf(buf, op, 1);
  K3_CHECK(buf.is_cuda(), "buffer must be on GPU");
  k3samd_kern::launch_atom_fill(at::hip::getCurrentHIPStream(), buf.data_ptr(),
                                slots, (int)op, seed);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void atom_gold(torch::Tensor buf, int64_t op, uint64_t seed, int64_t W) {
  K3_CHECK(k3samd_kern::atom_op_ok((int)op) && op == (int)op,
           "unknown atomics op id (see ops.ATOM_OPS)");
  const int64_t slots = check_atom_buf(buf, op, W);
  K3_CHECK(buf.is_cuda(), "buffer must be on GPU");
  k3samd_kern::launch_atom_gold(at::hip::getCurrentHIPStream(), buf.data_ptr(),
                                slots, (int)op, seed, (int)W);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void atom_reduce(torch::Tensor buf, int64_t op, uint64_t seed, int64_t W,
                 bool rotate, bool returning,
                 c10::optional<torch::Tensor> gold,
                 c10::optional<torch::Tensor> report, int64_t drop_w,
                 int64_t drop_tile) {
  check_atom_op(op, true);
  k3samd_kern::AtomReduceArgs a{};
  a.slots = check_atom_buf(buf, op, W);
  const int64_t tiles =
      (a.slots + k3samd_kern::kAtomTile - 1) / k3samd_kern::kAtomTile;
  K3_CHECK((drop_w == -1 && drop_tile == -1) ||
               (drop_w >= 0 && drop_w < W && drop_tile >= 0 &&
                drop_tile < tiles),
           "drop must be None or (w < W, tile < tiles)");
  K3_CHECK(returning == gold.has_value() && returning == report.has_value(),
           "returning=True needs gold and report; returning=False takes "
           "neither");
  if (returning) {
    K3_CHECK(gold->is_contiguous() &&
                 gold->element_size() == buf.element_size() &&
                 gold->numel() == buf.numel(),
             "gold must have the buffer's slot size and slot count");
    check_atom_report(*report, buf);
    K3_CHECK(gold->is_cuda() && gold->device() == buf.device(),
             "gold must be on the same GPU as the buffer");
    a.gold = gold->data_ptr();
    a.report = report->data_ptr();
  }
  K3_CHECK(buf.is_cuda(), "buffer must be on GPU");
  a.buf = buf.data_ptr();
  a.seed = seed;
  a.W = (int)W;
  a.rotate = rotate;
  a.drop_w = drop_w;
  a.drop_tile = drop_tile;
  k3samd_kern::launch_atom_reduce(at::hip::getCurrentHIPStream(), (int)op, a);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// `counters` must be zero; `where` int32 [ceil(draws / 256), 2].
void atom_ticket(torch::Tensor counters, torch::Tensor tickets,
                 torch::Tensor where) {
  const AtomTicketDims d = check_atom_ticket(counters, tickets);
  check_atom_where(where, k3samd_kern::atom_grid(d.draws), 1ll << 22);
  check_atom_ticket_devices(counters, tickets, where,
                            "where must be on the same GPU as the counters");
  k3samd_kern::launch_atom_ticket(at::hip::getCurrentHIPStream(), d.wide,
                                  counters.data_ptr(), d.counters,
                                  tickets.data_ptr(), d.draws,
                                  where.data_ptr());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// `perm` int32 [counters * ceil(draws / counters)], overwritten.
void atom_ticket_check(torch::Tensor counters, torch::Tensor tickets,
                       torch::Tensor perm, torch::Tensor report) {
  const AtomTicketDims d = check_atom_ticket(counters, tickets);
  K3_CHECK(perm.scalar_type() == torch::kInt32 && perm.is_contiguous() &&
               perm.numel() == k3samd_kern::atom_ticket_perm_words(d.draws,
                                                                   d.counters),
           "perm must be a contiguous int32 tensor of counters * "
           "ceil(draws / counters) elements");
  check_report_shape(report);
  check_atom_ticket_devices(counters, tickets, perm,
                            "perm must be on the same GPU as the counters");
  check_atom_report(report, counters);
  C10_HIP_CHECK(k3samd_kern::launch_atom_ticket_check(
      at::hip::getCurrentHIPStream(), d.wide, counters.data_ptr(), d.counters,
      tickets.data_ptr(), d.draws, perm.data_ptr(), report.data_ptr()));
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// One round of a chain op; `where` int32 [wgs, 2] sets the grid.
void atom_chain_round(torch::Tensor buf, int64_t op, uint64_t seed,
                      int64_t round, torch::Tensor report,
                      torch::Tensor where) {
  check_atom_op(op, false);
  const int64_t slots = check_atom_buf(buf, op, 1);
  K3_CHECK(round >= 0 && round < k3samd_kern::atom_w_cap((int)op),
           "round must be in 0 .. 4095");
  const int64_t wgs = check_atom_where(where, 0, k3samd_kern::kAtomMaxChainWgs);
  check_atom_report(report, buf);
  K3_CHECK(where.is_cuda() && where.device() == buf.device(),
           "where must be on the same GPU as the buffer");
  k3samd_kern::launch_atom_chain(at::hip::getCurrentHIPStream(), (int)op,
                                 buf.data_ptr(), slots, seed, (uint32_t)round,
                                 report.data_ptr(), where.data_ptr(), (int)wgs);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// Host code only (atom_pattern.h): bit patterns as unsigned integers.
void check_atom_pattern_args(int64_t op, int64_t w, int64_t W) {
  K3_CHECK(k3samd_kern::atom_op_ok((int)op) && op == (int)op,
           "unknown atomics op id (see ops.ATOM_OPS)");
  K3_CHECK(W >= 1 && W <= k3samd_kern::atom_w_cap((int)op) && w >= 0 && w < W,
           "0 <= w < W and 1 <= W <= the op's cap (240 packed, else 4096)");
}

uint64_t atom_init(int64_t op, uint64_t seed, uint64_t slot) {
  check_atom_pattern_args(op, 0, 1);
  return k3samd_kern::atom_init((int)op, seed, slot);
}

uint64_t atom_operand(int64_t op, uint64_t seed, uint64_t slot, int64_t w,
                      int64_t W) {
  check_atom_pattern_args(op, w, W);
  return k3samd_kern::atom_operand((int)op, seed, slot, (uint32_t)w,
                                   (uint32_t)W);
}

uint64_t atom_expected(int64_t op, uint64_t seed, uint64_t slot, int64_t W) {
  check_atom_pattern_args(op, 0, W);
  return k3samd_kern::atom_expected((int)op, seed, slot, (uint32_t)W);
}

bool atom_shape_ok(int64_t op, int64_t slots, int64_t W) {
  return op == (int)op && k3samd_kern::atom_shape_ok((int)op, slots, W);
}

std::vector<std::string> atom_op_names() {
  std::vector<std::string> names;
  for (int op = 0; op < k3samd_kern::kAtomOpCount; ++op)
    names.emplace_back(k3samd_kern::atom_op_name(op));
  return names;
}

// Host-side query: the extension only ships gfx950 code objects, so report
// whether the active device is gfx950.
bool has_mfma() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
  return std::string(prop.gcnArchName).find("gfx950") != std::string::npos;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("stream_triad", &stream_triad, "STREAM triad a = b + s*c (fp32)",
        py::arg("a"), py::arg("b"), py::arg("c"), py::arg("s"),
        py::arg("nontemporal") = false);
  m.def("stream_copy", &stream_copy, py::arg("a"), py::arg("b"),
        py::arg("nontemporal") = false);
  m.def("stream_scale", &stream_scale, py::arg("a"), py::arg("c"),
        py::arg("s"), py::arg("nontemporal") = false);
  m.def("stream_add", &stream_add, py::arg("a"), py::arg("b"), py::arg("c"),
        py::arg("nontemporal") = false);
  m.def("mfma_throughput", &mfma_throughput, py::arg("out"), py::arg("iters"),
        py::arg("shape") = 16);
  m.def("mfma_gemm16", &mfma_gemm16, py::arg("A"), py::arg("B"),
        py::arg("layout") = 0);
  m.def("mx_gemm16", &mx_gemm16, py::arg("A"), py::arg("B"),
        py::arg("fmt") = 0);
  m.def("has_mfma", &has_mfma);
  m.def("mem_fill", &mem_fill, py::arg("buf"), py::arg("pattern"),
        py::arg("seed"), py::arg("invert") = false,
        py::arg("cell_offset") = 0, py::arg("nontemporal") = true);
  m.def("mem_verify", &mem_verify, py::arg("buf"), py::arg("report"),
        py::arg("pattern"), py::arg("seed"), py::arg("invert") = false,
        py::arg("cell_offset") = 0);
  m.def("mem_verify_fill", &mem_verify_fill, py::arg("buf"),
        py::arg("report"), py::arg("old_pattern"), py::arg("old_seed"),
        py::arg("old_invert"), py::arg("new_pattern"), py::arg("new_seed"),
        py::arg("new_invert"), py::arg("cell_offset") = 0,
        py::arg("nontemporal") = true);
  m.def("gemm_fill", &gemm_fill, py::arg("buf"), py::arg("which"),
        py::arg("seed"), py::arg("rows"), py::arg("cols"));
  m.def("gemm_bf16_nt", &gemm_bf16_nt, py::arg("A"), py::arg("Bt"),
        py::arg("out") = py::none(), py::arg("where") = py::none());
  m.def("gemm_ref_int", &gemm_ref_int, py::arg("A"), py::arg("Bt"),
        py::arg("out") = py::none());
  m.def("gemm_dense_nt", &gemm_dense_nt, py::arg("A"), py::arg("Bt"),
        py::arg("out") = py::none(), py::arg("where") = py::none());
  m.def("gemm_dense_ref_int", &gemm_dense_ref_int, py::arg("A"), py::arg("Bt"),
        py::arg("out") = py::none());
  m.def("buf_compare", &buf_compare, py::arg("buf"), py::arg("expected"),
        py::arg("report"));
  m.def("mx_gemm16_scaled", &mx_gemm16_scaled, py::arg("A"), py::arg("SA"),
        py::arg("B"), py::arg("SB"), py::arg("fmt"));
  m.def("mx_fill", &mx_fill, py::arg("elems"), py::arg("scales"),
        py::arg("which"), py::arg("seed"), py::arg("rows"), py::arg("k"),
        py::arg("fmt"));
  m.def("mx_gemm_nt", &mx_gemm_nt, py::arg("A"), py::arg("SA"), py::arg("Bt"),
        py::arg("SB"), py::arg("fmt"), py::arg("out") = py::none(),
        py::arg("where") = py::none());
  m.def("mx_gemm_ref_int", &mx_gemm_ref_int, py::arg("A"), py::arg("SA"),
        py::arg("Bt"), py::arg("SB"), py::arg("fmt"),
        py::arg("out") = py::none());
  m.def("cu_lds_march", &cu_lds_march, py::arg("report"), py::arg("where"),
        py::arg("seed"), py::arg("passes") = 1, py::arg("stop_after") = 4,
        py::arg("inject") = py::none(), py::arg("dump") = py::none());
  m.def("cu_valu_signature", &cu_valu_signature, py::arg("report"),
        py::arg("where"), py::arg("seed"), py::arg("rounds"),
        py::arg("expected"), py::arg("sig_out") = py::none(),
        py::arg("inject") = py::none());
  m.def("cu_signature_expected", &cu_signature_expected, py::arg("seed"),
        py::arg("rounds"));
  m.def("link_pull_verify", &link_pull_verify, py::arg("host_buf"),
        py::arg("report"), py::arg("pattern"), py::arg("seed"),
        py::arg("invert") = false, py::arg("cell_offset") = 0,
        py::arg("wgs") = k3samd_kern::kLinkDefaultWgs);
  m.def("link_push_fill", &link_push_fill, py::arg("host_buf"),
        py::arg("pattern"), py::arg("seed"), py::arg("invert") = false,
        py::arg("cell_offset") = 0,
        py::arg("wgs") = k3samd_kern::kLinkDefaultWgs);
  m.def("link_duplex", &link_duplex, py::arg("pull_buf"), py::arg("report"),
        py::arg("pull_pattern"), py::arg("pull_seed"), py::arg("pull_invert"),
        py::arg("pull_cell_offset"), py::arg("push_buf"),
        py::arg("push_pattern"), py::arg("push_seed"), py::arg("push_invert"),
        py::arg("push_cell_offset"),
        py::arg("wgs") = 2 * k3samd_kern::kLinkDefaultWgs);
  m.def("link_chase", &link_chase, py::arg("host_buf"), py::arg("n"),
        py::arg("hops"), py::arg("out"));
  m.def("link_wall_clock_khz", &link_wall_clock_khz, py::arg("device"));
  m.def("link_host_fill", &link_host_fill, py::arg("buf"), py::arg("pattern"),
        py::arg("seed"), py::arg("invert") = false,
        py::arg("cell_offset") = 0, py::arg("threads") = 0);
  m.def("link_host_verify", &link_host_verify, py::arg("buf"),
        py::arg("pattern"), py::arg("seed"), py::arg("invert") = false,
        py::arg("cell_offset") = 0, py::arg("threads") = 0);
  m.def("link_chase_fill", &link_chase_fill, py::arg("buf"), py::arg("n"),
        py::arg("seed"));
  m.def("link_chase_expected", &link_chase_expected, py::arg("n"),
        py::arg("seed"), py::arg("hops"));
  m.def("atom_fill", &atom_fill, py::arg("buf"), py::arg("op"),
        py::arg("seed"));
  m.def("atom_gold", &atom_gold, py::arg("buf"), py::arg("op"),
        py::arg("seed"), py::arg("W"));
  m.def("atom_reduce", &atom_reduce, py::arg("buf"), py::arg("op"),
        py::arg("seed"), py::arg("W"), py::arg("rotate") = false,
        py::arg("returning") = false, py::arg("gold") = py::none(),
        py::arg("report") = py::none(), py::arg("drop_w") = -1,
        py::arg("drop_tile") = -1);
  m.def("atom_ticket", &atom_ticket, py::arg("counters"), py::arg("tickets"),
        py::arg("where"));
  m.def("atom_ticket_check", &atom_ticket_check, py::arg("counters"),
        py::arg("tickets"), py::arg("perm"), py::arg("report"));
  m.def("atom_chain_round", &atom_chain_round, py::arg("buf"), py::arg("op"),
        py::arg("seed"), py::arg("round"), py::arg("report"),
        py::arg("where"));
  m.def("atom_init", &atom_init, py::arg("op"), py::arg("seed"),
        py::arg("slot"));
  m.def("atom_operand", &atom_operand, py::arg("op"), py::arg("seed"),
        py::arg("slot"), py::arg("w"), py::arg("W"));
  m.def("atom_expected", &atom_expected, py::arg("op"), py::arg("seed"),
        py::arg("slot"), py::arg("W"));
  m.def("atom_shape_ok", &atom_shape_ok, py::arg("op"), py::arg("slots"),
        py::arg("W"));
  m.def("atom_op_names", &atom_op_names);
  m.attr("ATOM_REDUCE_OPS") = (int64_t)k3samd_kern::kAtomReduceOps;
  m.attr("LINK_DEFAULT_WGS") = (int64_t)k3samd_kern::kLinkDefaultWgs;
  m.attr("LINK_MAX_WGS") = (int64_t)k3samd_kern::kLinkMaxWgs;
  m.attr("MEM_REPORT_LEN") =(int64_t)k3samd_kern::kMemReportLen;
  m.attr("CU_LDS_BYTES") = (int64_t)k3samd_kern::kCuLdsBytes;
  m.attr("CU_LDS_CELLS") = (int64_t)k3samd_kern::kCuLdsCells;
  m.attr("CU_WG_THREADS") = (int64_t)k3samd_kern::kCuWgThreads;
  m.attr("CU_WAVES") = (int64_t)k3samd_kern::kCuWaves;
}
