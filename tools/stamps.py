"""Diagnostic: per-phase shader-clock shares of one batch from the -DMUSE_STAMPS build (never timed)."""
import sys, numpy as np, ctypes as C
sys.path.insert(0, __import__('os').path.dirname(__import__('os').path.dirname(__import__('os').path.abspath(__file__))))
import museinference_jl_amd as M
from museinference_jl_amd import build as B, _capi
B.LIB_PATH = B.LIB_PATH.replace("libmuse_hip.so", __import__("os").environ.get("MUSE_STAMPS_LIB", "libmuse_hip_stamps.so"))
lib = M.load_library()
N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
NTH = int(sys.argv[2]) if len(sys.argv) > 2 else 1
n = int(sys.argv[3]) if len(sys.argv) > 3 else 512
prob = M.HipMuseProblem(None, model="funnel", ntheta=NTH, N=N)
if len(sys.argv) > 4: prob.set_element_split(int(sys.argv[4]))
for _ in range(3): prob.map_and_score_batch(0,0,n,[1.0]*NTH)
lib.muse_debug_stamps(prob._ctx, C.c_int64(n), None)
prob.map_and_score_batch(0,0,n,[1.0]*NTH)
out = np.zeros((n,16), dtype=np.uint64)
lib.muse_debug_stamps(prob._ctx, C.c_int64(n), out.ctypes.data_as(C.c_void_p))
st = out[:, :8].astype(np.int64)
d = np.diff(st, axis=1)
names = ["sample/load", "eval0", "twoloop(s=-g)", "linesearch", "update", "(loop exit)", "score+zhat"]
print("median shader cycles per phase (wave 0):")
for k, nm in enumerate(names): print(f"  {nm:16s} {np.median(d[:,k]):10.0f}   ({np.median(d[:,k])/np.median(st[:,7]-st[:,0])*100:5.1f} %)")
ent = o0 = out.astype(np.int64)
last = (ent[:, 9] > st[:, 7]) & (ent[:, 9] - st[:, 7] < 10**7)
if last.any(): print("  last stamp of the last problem -> end of the kernel's loop: median", np.median(ent[last, 9] - st[last, 7]), "cycles over", int(last.sum()))
print("  sample detail: start->sampler loop end", np.median(out[:,8].astype(np.int64)-st[:,0]), " ->z init end", np.median(out[:,9].astype(np.int64)-out[:,8].astype(np.int64)), " ->barrier end", np.median(st[:,1]-out[:,9].astype(np.int64)))
o=out.astype(np.int64)
print("  line search detail: pre-logic", np.median(o[:,10]-st[:,3]), " eval1", np.median(o[:,11]-o[:,10]), " logic1", np.median(o[:,12]-o[:,11]), " eval2", np.median(o[:,13]-o[:,12]), " post-logic", np.median(st[:,4]-o[:,13]))
print("  final update pass: element loop", np.median(o[:,14]-st[:,4]), " reduction", np.median(o[:,15]-o[:,14]), " rest", np.median(st[:,5]-o[:,15]))
print("total per problem", np.median(st[:,7]-st[:,0]), "cycles; first start -> last end:", (st[:,7].max()-st[:,0].min()), "cycles")
# a workgroup's next problem starts right after its previous one ended (same CU, same counter): the smallest positive
# start - end distance of each problem to any other is the per-problem prologue/epilogue outside the stamped span
ends = np.sort(st[:, 7]); gaps = []
for s0 in st[:, 0]:
    k = np.searchsorted(ends, s0) - 1
    if k >= 0 and 0 < s0 - ends[k] < 20000: gaps.append(s0 - ends[k])
if gaps: print("between two problems of a workgroup (end stamp -> next start stamp): median", np.median(gaps), "cycles over", len(gaps), "pairs")
order = np.argsort(st[:,0]); 
print("start offsets of problems (cycles, sorted) sample:", (st[order,0]-st[:,0].min())[[0,1,n//5,n//2-1,n//2,n-1]])

# Detail mode (muse_debug_flags bit 10): slots 10-15 of a problem's row carry the map kernel's prologue and hand-over split instead
# of the line search's (csrc/kernels.hpp): 15 kernel entry, 10 kernarg words landed, 11 the barrier behind the LDS copy, 12
# load_problem_theta done -- first problem of a workgroup only --; 13, 14 the hand-over behind this problem (behind its first
# barrier / the next index known; a build whose hand-over has no barrier writes 14 only).  A launch of its own: same problems.
lib.muse_debug_flags(prob._ctx, 1024)
lib.muse_debug_stamps(prob._ctx, C.c_int64(n), None)
prob.map_and_score_batch(0,0,n,[1.0]*NTH)
lib.muse_debug_stamps(prob._ctx, C.c_int64(n), out.ctypes.data_as(C.c_void_p))
lib.muse_debug_flags(prob._ctx, 0)
o = out.astype(np.int64); st = o[:, :8]
med = lambda v: float(np.median(v)) if len(v) else float("nan")
first = (o[:, 15] > 0) & (o[:, 15] < st[:, 0]) & (st[:, 0] - o[:, 15] < 10**7)
print("prologue (detail launch, wave 0, shader cycles; median over", int(first.sum()), "workgroups):")
if first.any():
    f = o[first]
    print("  kernel entry -> kernarg words landed      ", med(f[:, 10] - f[:, 15]))
    print("  -> barrier behind the LDS copy            ", med(f[:, 11] - f[:, 10]))
    print("  -> pack_blocks, ticket, load_problem_theta", med(f[:, 12] - f[:, 11]))
    print("  -> begin()'s stamp 0 (describe)           ", med(f[:, 0] - f[:, 12]))
    print("  kernel entry -> first stamp of the workgroup's first problem: median", med(f[:, 0] - f[:, 15]), " min", int((f[:, 0] - f[:, 15]).min()), " max", int((f[:, 0] - f[:, 15]).max()))
print("  sample detail: start->sampler loop end", med(o[:, 8] - st[:, 0]), " ->start picked up (stamp 9)", med(o[:, 9] - o[:, 8]), " ->barrier end", med(st[:, 1] - o[:, 9]))
# hand-over: the problem that ended at stamp 7 of row q and the one whose stamp 0 follows it on the same compute unit
ends = np.argsort(st[:, 7]); ev = st[ends, 7]
rows = []
for r in range(n):
    k = np.searchsorted(ev, st[r, 0]) - 1
    if k >= 0 and 0 < st[r, 0] - ev[k] < 20000: rows.append((ends[k], r))
if rows:
    q = np.array([a for a, _ in rows]); r = np.array([b for _, b in rows])
    has13 = o[q, 13] > 0
    print("hand-over (detail launch; median over", len(rows), "pairs): end stamp -> next start stamp", med(st[r, 0] - st[q, 7]))
    if has13.any():
        print("  end stamp -> behind the first barrier", med(o[q[has13], 13] - st[q[has13], 7]), " -> next index known", med(o[q[has13], 14] - o[q[has13], 13]),
              " -> next stamp 0", med(st[r[has13], 0] - o[q[has13], 14]))
    else:
        print("  end stamp -> next index known", med(o[q, 14] - st[q, 7]), " -> next stamp 0", med(st[r, 0] - o[q, 14]))
