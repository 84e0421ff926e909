/* oracle/ref/shim/psapi.h -- TEST INFRASTRUCTURE ONLY.  Stand-in for <psapi.h>: the two translation units that
 * are built include it through viterbi.h and use nothing from it. */
