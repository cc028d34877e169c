// Common definitions for the inverse-audio-synthesis MI355X (gfx950) kernels.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IAS_HD __host__ __device__ __forceinline__
#else
// Host-only build of the per-sample arithmetic (used by tests/ to check the
// device math against the oracle without a GPU; never part of the product path).
#define IAS_HD inline
#endif

// Diagnostic switches.  The product library (libias_hip.so) has one kernel per operation and shape, reads NOTHING from
// the environment and keeps no mutable global state.  `make diag` builds libias_hip_diag.so from the same
// sources with -DIAS_DIAG, where the switches are live: scripts/diag, bench.py's `dxd` comparison figure, and the tests
// that compare a superseded kernel with its replacement load THAT library (inverse-audio-synthesis_amd/_lib.py:
// load_diag / use_library).  The split follows one rule:
//   kIasDiag        the one compile-time flag, true only under -DIAS_DIAG.
//   dispatch sites  a launch, hipFuncSetAttribute or occupancy query that ONLY a diagnostic switch can reach stands inside
//                   `if constexpr (kIasDiag) { ... }`, in one block in front of the product's choice, which follows as
//                   straight-line code.  A discarded statement instantiates nothing: the product build compiles neither
//                   the host stub nor the device code of a kernel template named only there: 262 kernels in the product
//                   library, 301 in the diagnostic one (tests/test_capi_symbols.py holds the inventory; scripts/isa_diff.py
//                   compares two source trees kernel by kernel).
//   ias_diag_env()  getenv in the diagnostic library, the constant NULL in the product library.  A switch that selects
//                   between kernels the product also reaches by shape or alignment stays such a runtime read: both
//                   kernels ship, and the product build folds the read away.
//   #ifdef IAS_DIAG only around DEFINITIONS the product build would otherwise emit or export: non-template __global__
//                   kernels, mutable globals, diagnostic-only extern "C" entry points, the matrix-core STFT's device
//                   code, and the superseded forms of cmul and its kin.  Never inside a launch if / else.
#ifdef IAS_DIAG
#include <stdlib.h>
constexpr bool kIasDiag = true;
static inline const char* ias_diag_env(const char* name) { return getenv(name); }
#else
constexpr bool kIasDiag = false;
#define ias_diag_env(name) ((const char*)0)
#endif

// The C ABI: every entry point, the IAS_OK / IAS_ERR_* status codes and struct IasReduceItem are declared once, in the
// public headers.  Every file that defines an entry point sees them through this include, so a definition whose
// parameter list differs from its declaration does not compile ("conflicting types"), and a kernel file that calls
// another file's entry point needs no declaration of its own.  Relative to this file: no compile line needs an -I.
#include "../../include/ias_hip.h"
#include "../../include/ias_hip_report.h"
#include "../../include/ias_hip_tied.h"
#include "../../include/ias_hip_gain.h"
#ifdef IAS_DIAG
#include "../../include/ias_hip_diag.h"
#endif

#define IAS_NPARAMS 78
// torchsynth LFO shape-mix exponent: LFO.__init__'s default `exponent = tensor(e)`, i.e. the fp32 0x402DF854
#define IAS_LFO_EXPONENT_F 2.7182817459106445f
#define IAS_NCTRL 5             // mod-matrix outputs: vco1 pitch, vco1 amp, vco2 pitch, vco2 amp, noise amp

// Per-voice scalars produced by the control-rate kernel, consumed at audio rate.
struct IasVoiceConst {
  float f0_1, depth_1, phi_1;   // vco_1: fl(midi_f0 + tuning), mod_depth, initial_phase
  float f0_2, depth_2, phi_2;   // vco_2
  float kpart;                  // fl(pi_f32 * partials_constant)
  float shape;                  // vco_2 shape
  float shape_gain;             // fl(1 - shape/2)
  float lvl0, lvl1, lvl2;       // mixer levels: vco_1, vco_2, noise
  float pad[4];
};
