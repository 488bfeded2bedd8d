// Compile check of coeb::CreateNewMapPointsNeighbors (adapter/LocalMapping_coeb.h) against reference-shaped
// types: new_map_points_exec.cpp without its main, so the templates are instantiated
// (tests/test_adapter_newpts.py, no GPU, no library).
#define main new_map_points_exec_main
#include "new_map_points_exec.cpp"
