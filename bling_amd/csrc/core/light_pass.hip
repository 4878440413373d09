// light_pass.hip -- host driver of one light tracer launch (Renderer/LightTracer.hs `pass`) over the
// kernel of light_tracer.h.
#include "core_internal.h"

namespace bcore {

template <uint32_t F>
uint32_t light_pass_t(bling_ctx* c, uint32_t seed, uint32_t pass, uint32_t first, uint32_t count, float* splat,
                      uint32_t rec_cap, bling_light_stats* st) {
  LightState& P = c->light;
  hipStream_t s = c->stream;
  if (P.ctr.n != 4) P.ctr.alloc(4);
  if (P.rec_count.n != 1) P.rec_count.alloc(1);
  if (rec_cap > 0 && P.rec.n < (size_t)2 * rec_cap) P.rec.alloc((size_t)2 * rec_cap);
  LtBufs B{};
  B.splat = splat;
  B.ctr = P.ctr.p;
  B.rec = rec_cap > 0 ? P.rec.p : nullptr;
  B.rec_count = P.rec_count.p;
  B.rec_cap = rec_cap;
  const EventPair ev;
  HIPCHK(hipMemsetAsync(P.ctr.p, 0, 4 * sizeof(unsigned long long), s));
  HIPCHK(hipMemsetAsync(P.rec_count.p, 0, sizeof(uint32_t), s));
  ev.a.record(s);
  if (count > 0) {
    k_lt_photon<F><<<(unsigned)(((uint64_t)count + 255) / 256), TRACE_BLOCK, c->lds_trace, s>>>(c->dscene.p, B, first, count,
                                                                                               seed, pass);
    HIPCHK(hipGetLastError());
  }
  ev.b.record(s);
  unsigned long long ctr[4];
  uint32_t nrec = 0;
  HIPCHK(hipMemcpyAsync(ctr, P.ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&nrec, P.rec_count.p, sizeof nrec, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (st) {
    st->photons = count;
    st->photon_rays = ctr[0]; st->shadow_rays = ctr[1]; st->splats = ctr[2]; st->dropped = ctr[3];
    st->ms_total = ev.elapsed_ms();
  }
  return nrec;
}

template uint32_t light_pass_t<kProfiles[0]>(bling_ctx*, uint32_t, uint32_t, uint32_t, uint32_t, float*, uint32_t,
                                             bling_light_stats*);
template uint32_t light_pass_t<kSppmAll>(bling_ctx*, uint32_t, uint32_t, uint32_t, uint32_t, float*, uint32_t,
                                         bling_light_stats*);

}  // namespace bcore
