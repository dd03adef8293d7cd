// tu_relocate.hip -- relocation candidates of lost features (ctr_relocate_device;
// relocate_kernels.h).  Every ellipse and every distance must round as NumPy's and
// cKDTree's do: no floating-point contraction anywhere in this unit.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "stage_common.h"
#include "locate_kernels.h"
#include "characterize_kernels.h"
#include "relocate_kernels.h"

template <typename T>
void launch_nd(int ndim, const RlArgs& a, size_t lds, hipStream_t s) {
  const dim3 grid((unsigned)a.n_queries), block(RL_THREADS);
  if (ndim == 2) hipLaunchKernelGGL((relocate_kernel<2, T>), grid, block, lds, s, a);
  else hipLaunchKernelGGL((relocate_kernel<3, T>), grid, block, lds, s, a);
}

}  // namespace

// The launch decision of the stage, all of it: the pixels of the LDS tile.  The kernel takes a
// query whose box has at most that many pixels in one slab, walks a larger one in slabs and reads
// one whose thinnest slab does not fit from global memory (relocate_kernels.h);
// tests/_relocate.py restates all three.
int ctr_relocate_launch(const ctr_relocate* r, StageRun* stage, const char** msg, long long* tile_pixels,
                        long long* lds_bytes) {
  *msg = "";
  if (!r) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (r->ndim != 2 && r->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (r->frame_dtype < CTR_DTYPE_U8 || r->frame_dtype > CTR_DTYPE_F64) { *msg = "unknown frame dtype"; return CTR_ERR_UNSUPPORTED; }
  if (r->n_frames < 0 || r->n_known < 0 || r->n_queries < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (!(r->scale_factor == r->scale_factor) || r->scale_factor == 0.) { *msg = "scale_factor must be a non-zero number"; return CTR_ERR_INVALID; }
  if (!(r->minmass == r->minmass)) { *msg = "minmass is NaN"; return CTR_ERR_INVALID; }
  if (r->max_candidates < 1) { *msg = "max_candidates must be >= 1"; return CTR_ERR_INVALID; }
  RlArgs a;
  const int nd = r->ndim;
  long long E = 1, one = 1, trailing = 1;
  double max_dist = 0.;
  a.sr_equal = 1;
  for (int d = 0; d < 3; ++d) {
    a.shape[d] = 1; a.radius[d] = 0; a.slice_radius[d] = 1; a.inv_slr2[d] = 1.; a.box[d] = 1; a.lo[d] = 0;
    a.sep[d] = 1.; a.inv_sep2[d] = 1.; a.sr[d] = 1.;
  }
  for (int d = 0; d < nd; ++d) {
    if (r->shape[d] < 1 || r->shape[d] > (1LL << 30)) { *msg = "frame shape must be in [1, 2^30]"; return CTR_ERR_INVALID; }
    if (r->radius[d] < 0) { *msg = "radius must be >= 0"; return CTR_ERR_INVALID; }
    if (r->radius[d] > 1024) { *msg = "radius above 1024"; return CTR_ERR_UNSUPPORTED; }
    const double sp = r->separation[d], sr = r->search_range[d];
    if (!(sp > 0.) || !(sp <= 1e6)) { *msg = "separation must be in (0, 1e6]"; return CTR_ERR_INVALID; }
    if (!(sr > 0.) || !(sr <= 1e6)) { *msg = "search_range must be in (0, 1e6]"; return CTR_ERR_INVALID; }
    E *= r->shape[d];
    if (E > 0x7fffffffLL) { *msg = "more than 2^31 - 1 pixels per frame"; return CTR_ERR_INVALID; }
    if (d > 0) trailing *= r->shape[d];
    a.shape[d] = (int)r->shape[d];
    a.radius[d] = (int)r->radius[d];
    a.sep[d] = sp;
    a.inv_sep2[d] = 1. / (sp * sp);
    a.sr[d] = sr;
    if (sr != r->search_range[0]) a.sr_equal = 0;
    // FindLinker.__init__ (find_link.py:766-781)
    const long long slr = (long long)(sr + (double)r->radius[d] + 1.);
    const long long bgr = slr + r->radius[d] + 1;
    a.slice_radius[d] = (int)slr;
    a.inv_slr2[d] = 1. / ((double)slr * (double)slr);
    max_dist = std::max(max_dist, (double)bgr / sr);
    one *= std::min<long long>(2 * slr + 1, r->shape[d]);
    // the dilation box as ctr_locate takes it: size 0 filters like size 1; a reach past the
    // frame's extent adds only the zero border, which a reach of the extent adds too
    long long b = (long long)(2. * sp / std::sqrt((double)nd));
    if (b < 1) b = 1;
    const long long lo = std::min<long long>((b - 1) / 2, r->shape[d]), hi = std::min<long long>(b / 2, r->shape[d]);
    a.box[d] = (int)(lo + hi + 1);
    a.lo[d] = (int)lo;
  }
  a.max_dist2 = max_dist * max_dist;
  // the tile: a one-source box, or the thinnest slab of a frame-wide box, whichever is larger
  static const long long elem[6] = {1, 2, 2, 4, 4, 8};
  const long long es = elem[r->frame_dtype], cap = CTR_RELOCATE_TILE_BYTES / es;
  const long long slab = std::min<long long>(a.box[0], r->shape[0]) * trailing;
  const long long tile = std::min(cap, std::max(one, slab));   // a slab beyond the cap: such boxes are read from global memory
  const long long lds = (tile * es + 15) & ~15LL;
  if (tile_pixels) *tile_pixels = tile;
  if (lds_bytes) *lds_bytes = lds;
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (r->n_queries > 0x7fffffffLL) { *msg = "too many queries for one call"; return CTR_ERR_INVALID; }
  if (r->n_queries > 0) {
    if (r->n_frames < 1 || !r->frames || !r->threshold || !r->known_offset) { *msg = "queries without frames, threshold or known_offset"; return CTR_ERR_INVALID; }
    if (r->n_known > 0 && !r->known_pos) { *msg = "null known_pos"; return CTR_ERR_INVALID; }
    if (!r->query_frame || !r->source_offset) { *msg = "null query_frame or source_offset"; return CTR_ERR_INVALID; }
    if (!r->n_found || !r->cand_pos || !r->mass || !r->signal || !r->size || !r->status) { *msg = "null output"; return CTR_ERR_INVALID; }
  }
  if (stage->mode != STAGE_LAUNCH || r->n_queries == 0) return CTR_OK;
  const hipStream_t s = stage->stream;
  a.frames = r->frames;
  a.frame_elems = E;
  a.n_frames = r->n_frames;
  a.isotropic = r->isotropic != 0;
  a.minmass = r->minmass;
  a.scale_factor = r->scale_factor;
  a.threshold = r->threshold;
  a.known_pos = r->known_pos;
  a.known_offset = (const long long*)r->known_offset;
  a.n_known = r->n_known;
  a.n_queries = r->n_queries;
  a.query_frame = (const long long*)r->query_frame;
  a.source_offset = (const long long*)r->source_offset;
  a.source_pos = r->source_pos;
  a.K = r->max_candidates;
  a.tile_elems = (int)tile;
  a.n_found = r->n_found;
  a.cand_pos = r->cand_pos;
  a.mass = r->mass;
  a.signal = r->signal;
  a.size = r->size;
  a.status = r->status;
  switch (r->frame_dtype) {
    case CTR_DTYPE_U8: launch_nd<uint8_t>(nd, a, (size_t)lds, s); break;
    case CTR_DTYPE_U16: launch_nd<uint16_t>(nd, a, (size_t)lds, s); break;
    case CTR_DTYPE_I16: launch_nd<int16_t>(nd, a, (size_t)lds, s); break;
    case CTR_DTYPE_I32: launch_nd<int32_t>(nd, a, (size_t)lds, s); break;
    case CTR_DTYPE_F32: launch_nd<float>(nd, a, (size_t)lds, s); break;
    default: launch_nd<double>(nd, a, (size_t)lds, s); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  return CTR_OK;
}
