/* Stands in for the CUDA runtime header in the host build of oracle/ref_build.py.
 * Everything the kernels need comes from ../cuda_on_cpu.h, which that build
 * force-includes. */
