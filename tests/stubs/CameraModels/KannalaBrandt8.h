// TEST INFRASTRUCTURE -- stand-in for the reference header of the same name: see standin_kb8.hpp.
#pragma once
#include "standin_kb8.hpp"
