// The plain LE / LEA kernel: any Q, any table layout, one thread per element.  The shard beyond the compiled latent widths (psi2_generic.hip), gp_predict with uncertain
// inputs and latent inference run it on views of their own tables; the arithmetic is varpoint.h's, as b_le_kernel (psi2.hip) spells it on its registers: one exponent on every path.
#include "gp_common.h"
#include "fexp.h"
#include "varpoint.h"
#include <algorithm>

namespace gp {

__global__ void __launch_bounds__(256) lea_rows_kernel(LeaRows a) {
  const long total = a.rows * a.Mp;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long n = e / a.Mp;
    const int m = (int)(e - n * a.Mp);
    if (a.mask && n < a.cnt && !a.mask[n]) continue;
    double le = kPadLog, lea = kPadLog;
    if (n < a.cnt && m < a.M) {
      double s, t;
      lea_sums(a.mu + n * a.ld, a.w + n * a.ld, a.v2 + n * a.ld, a.Z + m * a.ldz, a.Q, &s, &t);
      le = le_value(a.lnc2h[n * a.ldl], s);
      lea = lea_value(le, t);
    }
    if (a.LE) a.LE[e] = le;
    a.LEA[e] = lea;
  }
}

int launch_lea_rows(gp_ctx* c, hipStream_t st, const LeaRows& a) {
  GP_LAUNCH(c, st, lea_rows_kernel, dim3((unsigned)std::max<long>(1, std::min<long>((a.rows * a.Mp + 255) / 256, 16384))), dim3(256), 0, a);
  return GP_OK;
}

}  // namespace gp
