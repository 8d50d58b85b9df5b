/* Stand-in for the engine header of this name (test infrastructure only):
 * everything lives in standin.hpp. */
#pragma once
#include "standin.hpp"
