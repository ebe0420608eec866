/* the method codes of include/davidson_hip.h as a C caller gets them (tests/test_methods_cpu.py) */
#include <stdio.h>
#include "davidson_hip.h"
int main(void) {
  printf("%d %d %d %d %d %d %d %d\n", DAV_METHOD_DPR, DAV_METHOD_GJD, DAV_METHOD_NONE, DAV_METHOD_BDPR, DAV_METHOD_CHEB, DAV_METHOD_LCHEB,
         DAV_METHOD_CHEB_DEGREE(16), DAV_METHOD_LCHEB_DEGREE(16));
  return 0;
}
