/* Stands in for ATen in the host build of oracle/ref_build.py.  The at::Tensor
 * stub (sizes and a typed data pointer) is in ../../cuda_on_cpu.h, which that
 * build force-includes. */
