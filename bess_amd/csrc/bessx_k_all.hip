// bessx_k_all.hip -- all device translation units as ONE, for the instrumented builds (make ktrace / make prof): their
// time stamps and counters live in __device__ variables of bessx_kdev.hpp, which every separately compiled unit would
// own a copy of.  Never part of the product library.
#include "bessx_k_lm.hip"
#include "bessx_k_ingest.hip"
#include "bessx_k_predict.hip"
#include "bessx_k_eval.hip"
#include "bessx_k_coxeval.hip"
#include "bessx_k_coxsurv.hip"
#include "bessx_k_info.hip"
#include "bessx_k_diag.hip"
#include "bessx_k_sandwich.hip"
#include "bessx_k_coxinfo.hip"
#include "bessx_k_coxdiag.hip"
#include "bessx_k_solve.hip"
#include "bessx_k_glm.hip"
#include "bessx_k_cox.hip"
#include "bessx_k_cov.hip"
#include "bessx_cgbig.hip"
