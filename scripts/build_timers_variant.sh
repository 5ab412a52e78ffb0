# Profiling build of the device library with the per-phase shader-clock counters compiled in (the product build
# compiles them out, wave.h). Used by scripts/gpu_quick.sh; never loaded by the product. Every translation unit of the
# library, as build() compiles them (the pack kernels live in units of their own: ksolve.hip alone does not link).
cd "$(dirname "$0")/.." && mkdir -p karpenter_amd/variants && \
  python -c "import __graft_entry__ as g; g.build_ksolve('karpenter_amd/variants/libksolve_timers.so', defines=('-DKSOLVE_PHASE_TIMERS',))"
