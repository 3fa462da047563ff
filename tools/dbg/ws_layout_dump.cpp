// Prints the byte offset of every member of every workspace libipmz carves
// (DESIGN.md "Workspaces"), from a fake base that is never dereferenced, and
// the totals.  Host only: no HIP device call.  Built by `make wsdump` against
// the product objects; its output for this tree and for the tree before the
// carving was unified are profiles/capi_ws/layout_new.txt / layout_parent.txt
// (identical files: callers allocate by the *_workspace_bytes functions and
// the tests index the mixed workspace directly, so no member may move).
#include <cstdio>

#include "capi.h"

static char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 40);

// offset of p, -1 for a member the layout does not have
static long long off(const void* p) { return p ? (long long)(static_cast<const char*>(p) - BASE) : -1; }

static void dump_ldlt(int N, int nbi, int nbo) {
  const LdltWs w = ldlt_ws(BASE, N, nbo, nbi);
  printf("ldlt N=%d nbi=%d nbo=%d info=%lld pctrl=%lld side=%lld Linv=%lld W=%lld y=%lld z=%lld ctrl=%lld P=%lld "
         "total=%lld size_only=%lld\n",
         N, nbi, nbo, off(w.info), off(w.pctrl), off(w.side), off(w.Linv), off(w.W), off(w.y), off(w.z), off(w.ctrl),
         off(w.P), (long long)w.total, (long long)ldlt_ws(nullptr, N, nbo, nbi).total);
}

static void dump_mixed(int N, int nbo) {
  MixedWs w;
  const long long total = mixed_ws_carve(BASE, N, nbo, w);
  printf("mixed N=%d nbo=%d ld32=%lld K32=%lld D32=%lld Linv32=%lld W32=%lld y32=%lld z32=%lld r32=%lld ctrl=%lld "
         "P32=%lld state=%lld info=%lld pctrl=%lld s=%lld x=%lld colp=%lld rowp=%lld part=%lld stat=%lld total=%lld "
         "bytes=%lld\n",
         N, nbo, (long long)w.ld32, off(w.K32), off(w.D32), off(w.Linv32), off(w.W32), off(w.y32), off(w.z32),
         off(w.r32), off(w.ctrl), off(w.P32), off(w.state), off(w.info), off(w.pctrl), off(w.s), off(w.x), off(w.colp),
         off(w.rowp), off(w.part), off(w.stat), total, (long long)mixed_ws_bytes(N, nbo));
}

static void dump_mixed_multi(int N, int nrhs) {
  MixedMultiWs m;
  const long long total = mixed_multi_ws_carve(BASE, N, nrhs, m);
  MixedMultiWs m0;
  printf("mixed_multi N=%d nrhs=%d ldx=%lld ld32=%lld ntiles=%d x=%lld r32=%lld part=%lld stat=%lld done=%lld "
         "word=%lld total=%lld size_only=%lld\n",
         N, nrhs, (long long)m.ldx, (long long)m.ld32, m.ntiles, off(m.x), off(m.r32), off(m.part), off(m.stat),
         off(m.done), off(m.word), total, (long long)mixed_multi_ws_carve(nullptr, N, nrhs, m0));
}

static void dump_normal(int n, int mp) {
  ipmz_ctx ctx;  // the default blocking
  const NormalWs w = normal_ws(BASE, n + mp, nbo_for(&ctx, n + mp), ctx.nbi);
  printf("normal n=%d mp=%d info=%lld k.info=%lld k.pctrl=%lld k.side=%lld k.Linv=%lld k.W=%lld k.y=%lld k.z=%lld "
         "k.ctrl=%lld k.P=%lld total=%lld\n",
         n, mp, off(w.info), off(w.k.info), off(w.k.pctrl), off(w.k.side), off(w.k.Linv), off(w.k.W), off(w.k.y),
         off(w.k.z), off(w.k.ctrl), off(w.k.P), (long long)w.total);
}

static void dump_bk(int N) {
  const BkWs w = bk_ws(BASE, N);
  printf("bk_ws N=%d Linv=%lld P=%lld y=%lld x=%lld ctrl=%lld meta=%lld total=%lld size_only=%lld\n", N, off(w.Linv),
         off(w.P), off(w.y), off(w.x), off(w.ctrl), off(w.meta), (long long)w.total, (long long)bk_ws(nullptr, N).total);
  printf("bk_meta N=%d flag=%lld ones=%lld tmp=%lld total=%lld\n", N, off(bk_fast_flag(BASE)), off(bk_fast_ones(BASE, N)),
         off(bk_fast_tmp(BASE, N)), (long long)bk_fast_meta_bytes(N));
}

int main() {
  const int Ns[] = {1, 63, 64, 65, 129, 320, 1000, 2047, 2048, 2560, 4096, 4097, 11264, 16384};
  for (int N : Ns)
    for (int nbi : {64, 128})
      for (int nbo : {nbi, 256, 384, 512}) dump_ldlt(N, nbi, nbo);
  for (int N : Ns)
    for (int nbo : {128, 256, 384, 512}) dump_mixed(N, nbo);  // (128: ipmz_ctx_set_blocking(128, 128))
  for (int N : Ns)
    for (int nrhs : {1, 2, 7, 8, 64, 257}) dump_mixed_multi(N, nrhs);
  dump_normal(64, 0);
  dump_normal(100, 37);
  dump_normal(2048, 512);
  for (int N : Ns) dump_bk(N);
  return 0;
}
