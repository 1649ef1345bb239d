/*
 * fixed_class.h -- stand-in for the 16.16 fixed-point class header the reference includes but does not ship.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/Makefile, target `ref`).  The reference is built with USING_FIXED_POINT false, so all it
 * needs from this header in that mode is a type called fixed_point<p> with an intValue member that can be made from a double
 * or an int (two locals of its main(), which the harness never calls), and the name `fixed`.  No arithmetic is defined: the
 * float path never does any on this type, and a use of one would be a compile error rather than a silent guess.
 */
#ifndef ORACLE_REF_FIXED_CLASS_H_
#define ORACLE_REF_FIXED_CLASS_H_

template <int p>
struct fixed_point {
    int intValue;
    fixed_point() : intValue(0) {}
    fixed_point(double v) : intValue((int)(v * (double)(1 << p))) {}
    fixed_point(int v) : intValue(v << p) {}
};

typedef fixed_point<16> fixed;

#endif /* ORACLE_REF_FIXED_CLASS_H_ */
