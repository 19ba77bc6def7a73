// mvs_patch.hip -- the translation unit of every kernel that runs the patch arithmetic of mvs_device.cuh / mvs_check.cuh (sampling,
// refinement, setRefImage, Optim::check).  The sources are cut by concern into three files, each with its kernels and their launchers:
//   mvs_sweep.cuh    the job lists, the sweep with its retry tier, the choice of a launch's kernel variant, the commit of a pass
//   mvs_filter.cuh   pool upkeep (k_fill_ncc among it) and Filter::run
//   mvs_probe.cuh    the probes
// They are compiled as ONE unit, in this order, because the machine code of these kernels depends on which other users of the shared
// inline functions the compiler meets in the unit: compiled alone, k_fill_ncc, k_filter_outside, k_filter_exact, k_probe and
// k_probe_refine come out with another schedule and other registers (profiles/r24_codeobj_kernel_split.txt), and these kernels sit at
// their register limits.  Whoever makes one of the three a unit of its own starts from a measured A/B of the kernels that change.
#include "mvs_sweep.cuh"
#include "mvs_filter.cuh"
#include "mvs_probe.cuh"
