// Compile check of the keyframe-database adapter (adapter/KeyFrameDatabase_coeb.h) against
// reference-shaped types and DBoW2-shaped containers: kfdb_exec.cpp without its main, so the
// templates are instantiated (tests/test_adapter_kfdb.py, no GPU, no library).
#define main kfdb_exec_main
#include "kfdb_exec.cpp"
