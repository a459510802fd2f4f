// user_model.hpp -- a USER-SUPPLIED elementwise model (include/muse_model.h; the reference's SimpleMuseProblem closures,
// src/simple.jl:79-95, as compiled code).  When the library is built with -DMUSE_USER_MODEL_HEADER="<header>" the header's
// three functions are compiled for the device (models.hpp wraps them as UserModel<MAXB>, which the solver kernel is
// instantiated with exactly like a built-in model) and for the host (muse_engine.cpp checks the contract's zero-element
// requirements when a context is created).  Such a library holds ONLY the user model (model id MUSE_MODEL_USER).
#pragma once
#ifdef MUSE_USER_MODEL_HEADER
#include <math.h>
#if defined(__HIPCC__)
#define MUSE_MODEL_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define MUSE_MODEL_FN static inline
#endif
// where a launch's run-time constants sit in its kernel-argument block (args.hpp, BatchArgs::consts; muse_model.h, muse_const)
#include "args.hpp"
#define MUSE_KERNARG_CONSTS (muse::kArgsConstsOffset)
// what a header forms exponentials with (include/muse_model.h): the engine's exp -- one fixed sequence of IEEE operations, the same
// on host and device (step.hpp) and in the CPU checker.  In device code the header's PER-ELEMENT functions get muse::model_exp
// (model_math.hpp: the same bits for every argument from a branch-free sequence the resident solve has the registers for);
// muse_model_coefs -- once per theta, in the step of the loop kernel -- keeps muse::muse_exp there too, told apart by the name of
// the function the macro is expanded in (a comparison of two string constants: folded at compile time).  The consequence for a
// header's author: only the text of muse_model_coefs ITSELF keeps muse_exp on the device -- a helper function of the header that
// muse_model_coefs calls gets model_exp like every other function.  The bits are the same either way; what changes is the loop
// kernel's code (its step inlines the helper), hence its resource rows.
// -DMUSE_MODEL_EXP_PLAIN maps everything to muse::muse_exp as the host does: the build tools/model_exp_bench.py compares with.
#include "step.hpp"
#include "model_math.hpp"
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MUSE_MODEL_EXP_PLAIN)
namespace muse {
constexpr bool in_model_coefs(const char* f) {
    const char* n = "muse_model_coefs";
    while (*n && *f == *n) ++f, ++n;
    return *f == *n;
}
}  // namespace muse
#define muse_model_exp(x) (muse::in_model_coefs(__func__) ? muse::muse_exp(x) : muse::model_exp(x))
#else
#define muse_model_exp(x) muse::muse_exp(x)
#endif
#include MUSE_USER_MODEL_HEADER
#ifndef MUSE_MODEL_NAME
#error "the model header must #define MUSE_MODEL_NAME (include/muse_model.h)"
#endif
#endif
