/*
 * ref_shim.hpp -- force-included (-include) into every translation unit of the
 * reference (LLNL/graph-embed: src/partitioner.cpp, src/embed.cpp,
 * src/matrixutils.cpp and, through them, include/forceatlas.hpp) and into
 * ref_driver.cpp when oracle/Makefile builds oracle/_ref/ge_ref.
 *
 * TEST INFRASTRUCTURE ONLY.  It supplies the two things the reference's own
 * files expect from their surroundings and do not name themselves:
 *
 *   1. the standard headers the real linalgcpp.hpp pulls in before the
 *      reference's code is seen;
 *   2. a deterministic std::random_device.  The reference seeds each mt19937
 *      with rd(); here rd() returns the process-wide ge_ref_seed, so every
 *      generator starts from the seed the caller chose -- the convention
 *      ge_oracle.h pins ("every RNG is std::mt19937(seed)").
 *
 * No line of the reference is restated here.
 */
#ifndef GE_REF_SHIM_HPP
#define GE_REF_SHIM_HPP

#include <algorithm>
#include <cassert>
#include <cmath>
#include <functional>
#include <iostream>
#include <map>
#include <numeric>
#include <random>
#include <set>

extern unsigned ge_ref_seed;

namespace std {
struct ge_ref_random_device {
  typedef unsigned int result_type;
  result_type operator()() { return ge_ref_seed; }
};
}  // namespace std

/* after <random>, so the library's own class keeps its name */
#define random_device ge_ref_random_device

#endif
