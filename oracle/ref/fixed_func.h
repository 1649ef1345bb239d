/*
 * fixed_func.h -- stand-in for the fixed-point helper header the reference includes but does not ship.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/Makefile, target `ref`).  In float mode the reference names one function of it, in a
 * diagnostic print of its main(): fix2float<p>(int), the value of a p-fractional-bit integer.
 */
#ifndef ORACLE_REF_FIXED_FUNC_H_
#define ORACLE_REF_FIXED_FUNC_H_

template <int p>
inline float fix2float(int v) { return (float)v / (float)(1 << p); }

#endif /* ORACLE_REF_FIXED_FUNC_H_ */
