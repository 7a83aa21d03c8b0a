// aset_reduce.h -- a stub, comments only.  This file held the device functions of the active-set iteration for the warm QP
// solves, an experiment that was measured, rejected and retired from the tree (DESIGN.md sections 3.3 and 7;
// tests/tools/qp_active_set_study.py states the method in numpy and is its record).  Nothing includes this file.  It keeps its
// name because bench.py lists it among the sources of the QP kernels (_QP_SRC) and hashes those files by name to decide whether
// a counter record of profiles/ is current when the LLVM tools that fingerprint the machine code are absent; a missing file
// there is an error, and how the benchmark measures is not for a change of the product to edit.
