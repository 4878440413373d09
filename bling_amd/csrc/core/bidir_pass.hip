// bidir_pass.hip -- host driver of one wave of the bidirectional path integrator
// (Integrator/BidirPath.hs) over the kernels of bidir.h.
//
// The kernels exist for two feature sets: the cornell profile, compiled here with the driver, and
// every feature (FT_ALL, computed textures included), whose walk and connection kernels compile in
// units of their own -- bidir_pass_walk.hip and bidir_pass_connect.hip include this file with
// BLING_BIDIR_UNIT_WALK_ALL / BLING_BIDIR_UNIT_CONNECT_ALL set -- so the build runs them side by side.
#include "core_internal.h"

namespace bcore {

template <uint32_t F>
void bidir_walk_launch(bling_ctx* c, const WaveState& W, const BdBufs& B, const TileDesc* tiles, unsigned n_tiles,
                       uint32_t max_tile, const int32_t* list, uint32_t n, uint32_t seed, uint32_t pass) {
  const dim3 gw = tiles ? dim3((max_tile + 255) / 256, n_tiles) : dim3((n + 255) / 256, 1);
  k_bd_walk<F><<<gw, TRACE_BLOCK, c->lds_trace, c->stream>>>(c->dscene.p, W, B, tiles, list, n, seed, pass, c->counters.p);
}

template <uint32_t F>
void bidir_connect_launch(bling_ctx* c, const BdBufs& B, uint32_t n) {
  const uint64_t lanes = (uint64_t)n * (uint64_t)B.md;               // one per (sample, light vertex)
  k_bd_connect<F><<<(unsigned)((lanes + 255) / 256), TRACE_BLOCK, c->lds_trace, c->stream>>>(c->dscene.p, B, n, c->counters.p);
}

#define BLING_BD_WALK_ARGS bling_ctx*, const WaveState&, const BdBufs&, const TileDesc*, unsigned, uint32_t, const int32_t*, \
                           uint32_t, uint32_t, uint32_t
#if defined(BLING_BIDIR_UNIT_WALK_ALL)
template void bidir_walk_launch<FT_ALL>(BLING_BD_WALK_ARGS);
#elif defined(BLING_BIDIR_UNIT_CONNECT_ALL)
template void bidir_connect_launch<FT_ALL>(bling_ctx*, const BdBufs&, uint32_t);
#else
extern template void bidir_walk_launch<FT_ALL>(BLING_BD_WALK_ARGS);
extern template void bidir_connect_launch<FT_ALL>(bling_ctx*, const BdBufs&, uint32_t);

BdBufs bidir_bufs(bling_ctx* c, uint32_t n, float* terms) {
  BidirState& P = c->bidir;
  if (P.md != c->S.max_depth || P.md < 1 || P.md > BD_MAX_DEPTH || n > P.cap)
    throw std::runtime_error("bidir vertex buffers do not fit the wave");
  BdBufs B{};
  B.vorg = P.vorg.p; B.vdir = P.vdir.p; B.vhit = P.vhit.p; B.vwo = P.vwo.p; B.valpha = P.valpha.p;
  B.ld = P.ld.p; B.conn = P.conn.p; B.le = P.le.p; B.info = P.info.p;
  B.terms = reinterpret_cast<float4*>(terms);
  B.cap = P.cap; B.md = P.md;
  return B;
}

void bidir_connect_finish(bling_ctx* c, const WaveState& W, const BdBufs& B, uint32_t n) {
  if ((c->features & ~kProfiles[0]) == 0u) bidir_connect_launch<kProfiles[0]>(c, B, n);
  else bidir_connect_launch<FT_ALL>(c, B, n);
  k_bd_finish<<<(n + 255) / 256, 256, 0, c->stream>>>(W, B, n, c->counters.p);
  HIPCHK(hipGetLastError());
}

int bidir_wave(bling_ctx* c, const WaveState& W, const TileDesc* tiles, unsigned n_tiles, uint32_t max_tile,
               const int32_t* list, uint32_t n, uint32_t seed, uint32_t pass, float* terms) {
  if (n == 0) return 0;
  const BdBufs B = bidir_bufs(c, n, terms);
  if ((c->features & ~kProfiles[0]) == 0u) bidir_walk_launch<kProfiles[0]>(c, W, B, tiles, n_tiles, max_tile, list, n, seed, pass);
  else bidir_walk_launch<FT_ALL>(c, W, B, tiles, n_tiles, max_tile, list, n, seed, pass);
  bidir_connect_finish(c, W, B, n);
  return 3;
}
#endif

}  // namespace bcore
